"""The cases, references and bars of tests/monodepth_cases.py, checked without a GPU and without the library: the tables against what each
case claims to reach, the conditions on the inputs that keep the discontinuities out (fragile, clipped, unjudged shares), the fp32 torch
composition under RHO32 (which fixes kappa), the restated samplers against torch's, and the thirteen defects the bars must see."""
import pytest
import torch
import torch.nn.functional as F

import monodepth_cases as MC

_VS, _PH = {}, {}


def _vs(run):
    """(t, cond, r64) of a view-synthesis run: computed once and left unchanged."""
    if run not in _VS:
        t, cond = MC.vs_inputs(run)
        _VS[run] = (t, cond, MC.vs_reference(t, MC.VS_BY_ID[run[0]], run[1]))
    return _VS[run]


def _ph(cid):
    """(t, forward r64, {map name: (argmin map, grad_color r64)}) of a photometric case."""
    if cid not in _PH:
        case = MC.PH_BY_ID[cid]
        t = MC.ph_inputs(case)
        f64 = MC.ph_forward(t, case)
        maps = {w: MC.ph_argmin_map(case, w, f64["argmin"]) for w in MC.ph_maps(case)}
        _PH[cid] = (t, f64, {w: (m, MC.ph_backward(t, case, m)) for w, m in maps.items()})
    return _PH[cid]


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    _VS.clear()
    _PH.clear()
    _RHO.clear()
    MC._VS_INPUTS.clear()


def test_tables_are_well_formed():
    for table in (MC.VS_CASES, MC.PH_CASES):
        ids = [c["id"] for c in table]
        assert len(set(ids)) == len(ids)
    for c in MC.VS_CASES:
        assert 1 <= c["S"] <= 4 and 1 <= c["NF"] <= 2 and c["H"] >= 2 and c["W"] >= 2, c["id"]
        assert c["H"] % (1 << (c["S"] - 1)) == 0 and c["W"] % (1 << (c["S"] - 1)) == 0, c["id"]
        assert c["S"] * c["NF"] * c["B"] * c["H"] * c["W"] <= 8192, c["id"]            # a few thousand pixels: every GPU test runs in well under a second
    for c in MC.PH_CASES:
        assert 1 <= c["S"] <= 4 and 1 <= c["NF"] <= 2 and c["H"] >= 2 and c["W"] >= 2, c["id"]
        assert c["S"] * c["NF"] * c["B"] * c["H"] * c["W"] <= 16384, c["id"]
    assert len(set(MC.VS_RUNS)) == len(MC.VS_RUNS)
    for runs, _ in MC.VS_DEFECTS.values():
        assert set(runs) <= set(MC.VS_RUNS)
    for cids, _ in MC.PH_DEFECTS.values():
        assert set(cids) <= set(MC.PH_BY_ID)
    assert len(MC.DEFECTS) == 13


def test_view_synthesis_table_reaches_what_it_names():
    C = MC.VS_BY_ID
    px = lambda c: c["H"] * c["W"]
    assert (C["min2x2"]["H"], C["min2x2"]["W"], C["min2x2"]["S"], C["min2x2"]["NF"]) == (2, 2, 1, 1)
    assert px(C["s3-b3"]) < 256 and MC.vs_blocks(C["s3-b3"]) == 1                       # one partly filled block
    assert px(C["one-block"]) == 256 and MC.vs_blocks(C["one-block"]) == 1 and C["one-block"]["NF"] == 1
    assert 256 < px(C["odd-s1"]) < 320 and MC.vs_blocks(C["odd-s1"]) == 2               # just above one block
    assert px(C["ragged-2blk"]) == 320 and MC.vs_blocks(C["ragged-2blk"]) == 2 and px(C["ragged-2blk"]) % MC.VS_THREADS != 0
    assert MC.vs_blocks(C["wide"]) == 3 and px(C["wide"]) % MC.VS_THREADS != 0
    assert (C["s3-1x1"]["H"] >> 3, C["s3-1x1"]["W"] >> 3) == (1, 1) and C["s3-1x1"]["S"] == 4         # up_index with n = 1 both ways
    assert (C["wide"]["H"] >> 3, C["wide"]["W"] >> 3) == (1, 9) and C["wide"]["S"] == 4
    for c in MC.VS_REFUSED:                                                             # outside the contract for one reason alone
        assert c["H"] % 8 == 0 and c["W"] % (1 << (c["S"] - 1)) != 0 and c["W"] % 2 == 0
    assert (C["s3-b3"]["S"], C["s3-b3"]["B"], C["s3-b3"]["NF"]) == (3, 3, 2)
    assert C["odd-s1"]["H"] % 2 == 1 and C["odd-s1"]["W"] % 2 == 1 and C["odd-s1"]["S"] == 1
    assert {c["S"] for c in MC.VS_CASES} >= {1, 3, 4} and {c["NF"] for c in MC.VS_CASES} == {1, 2}
    # K, inv_K and cam_T_cam differ per item
    t = MC.vs_raw_inputs(C["s3-b3"])
    assert len({tuple(k.flatten().tolist()) for k in t["K"]}) == 3 and len({tuple(m.flatten().tolist()) for m in t["T"].flatten(0, 1)}) == 6
    # every case in all three modes; mode 1 and mode 2 with gres all given, all NULL and partly NULL
    for c in MC.VS_CASES:
        if not c["behind"]:
            assert {m for cid, m, _ in MC.VS_RUNS if cid == c["id"]} == {0, 1, 2}
    for m in (1, 2):
        assert {g for _, mm, g in MC.VS_RUNS if mm == m} == {"all", "none", "some"}
    given = MC.gres_given(C["ragged-2blk"], "some")
    assert any(given) and not all(given)
    assert ("behind", 0, "none") in MC.VS_RUNS


def test_photometric_table_reaches_what_it_names():
    C = MC.PH_BY_ID
    assert MC.ph_tiles(C["one-tile"]) == (1, 1) and (C["one-tile"]["H"], C["one-tile"]["W"]) == (MC.PH_TY, MC.PH_TX)
    assert MC.ph_tiles(C["edge-tiles"]) == (2, 2) and C["edge-tiles"]["H"] % MC.PH_TY == 1 and C["edge-tiles"]["W"] % MC.PH_TX == 1
    assert MC.ph_tiles(C["sub-tile"]) == (1, 1) and C["sub-tile"]["H"] < MC.PH_TY and C["sub-tile"]["W"] < MC.PH_TX
    assert MC.ph_tiles(C["seams"]) == (2, 2) and C["seams"]["H"] % MC.PH_TY == 0 and C["seams"]["W"] % MC.PH_TX == 0 and C["seams"]["S"] == 4
    assert MC.ph_tiles(C["wide-short"]) == (3, 1) and C["wide-short"]["H"] == 3 and C["wide-short"]["B"] == 3
    assert (C["min2x2"]["H"], C["min2x2"]["W"]) == (2, 2) and (C["refl3x3"]["H"], C["refl3x3"]["W"]) == (3, 3)
    assert {c["H"] % MC.PH_TY != 0 for c in MC.PH_CASES} == {False, True}                              # partial tiles in y at last
    assert {c["S"] for c in MC.PH_CASES} == {1, 2, 3, 4} and {c["automask"] for c in MC.PH_CASES} == {0, 1}
    # in the table's main cases every candidate wins somewhere
    for cid in ("one-tile", "seams", "sub-tile"):
        _, f64, _ = _ph(cid)
        assert set(f64["argmin"].flatten().tolist()) == set(range(2 * C[cid]["NF"])), cid
    # the flat patch: candidate 0 and target bit-identical on a block -> value exactly 0 wherever the whole window lies inside, selected
    t, f64, _ = _ph("flat-patch")
    assert torch.equal(t["color"][0, 0, :, :, 2:9, 5:37], t["target"][:, :, 2:9, 5:37])
    assert bool((f64["values"][0, 0, :, 3:8, 6:36] == 0).all()) and bool((f64["argmin"][0, :, 3:8, 6:36] == 0).all())
    # the designed ties: bit-identical candidates, so exactly equal values, and the first wins everywhere
    for cid in ("tie-warped", "tie-identity"):
        t, f64, _ = _ph(cid)
        assert torch.equal(f64["values"][:, 0], f64["values"][:, 1]) and not bool(f64["argmin"].any()), cid
    t, _, _ = _ph("tie-identity")
    assert not bool(t["noise"].any()) and torch.equal(t["color"][0], t["src"]) and torch.equal(t["color"][1], t["src"])
    t, _, _ = _ph("tie-warped")
    assert torch.equal(t["color"][:, 0], t["color"][:, 1])


@pytest.mark.parametrize("run", MC.VS_RUNS, ids=MC.vs_run_id)
def test_view_synthesis_inputs_keep_their_conditions(run):
    case = MC.VS_BY_ID[run[0]]
    t, cond, r64 = _vs(run)
    print(MC.vs_run_id(run), cond)
    assert cond["fragile"] <= MC.MAX_FRAGILE and cond["min_abs_z"] >= MC.MIN_ABS_Z, cond
    if case["H"] * case["W"] >= 256:
        assert cond["clipped"] >= MC.MIN_CLIPPED and cond["unclipped"] >= MC.MIN_UNCLIPPED, cond
    live = r64["A_gT"] > 0
    cancel = float((r64["A_gT_channels"][live] / r64["A_gT"][live]).max()) if bool(live.any()) else 1.0
    print(MC.vs_run_id(run), "largest channel cancellation of a cam_T_cam element:", round(cancel, 2))
    assert cancel <= MC.MAX_CHANNEL_CANCELLATION, cancel
    assert (cond["behind"] > 0) == case["behind"], cond                                # a few points behind the camera, in that case alone
    if case["behind"]:
        assert cond["behind"] <= 0.25 * case["NF"] * case["B"] * case["H"] * case["W"]
    for a in t["disp"]:
        assert 0.0199 <= float(a.min()) and float(a.max()) <= 0.6001
    assert 0.1 <= float(t["src"].min()) and float(t["src"].max()) <= 0.9001
    assert [g is not None for g in t["gres"]] == (MC.gres_given(case, run[2]) if run[1] else [False] * (case["S"] * case["NF"]))
    for n in MC.vs_outputs(run[1]):
        for a in (r64[n] if isinstance(r64[n], list) else [r64[n]]):
            assert bool(a.isfinite().all()), n


@pytest.mark.parametrize("cid", [c["id"] for c in MC.PH_CASES])
def test_photometric_inputs_keep_their_conditions(cid):
    case = MC.PH_BY_ID[cid]
    t, f64, maps = _ph(cid)
    unjudged = 1.0 - float(MC.judged_pixels(f64).double().mean())
    print(cid, "unjudged share:", unjudged)
    if case["special"] not in ("tie_warped", "tie_identity") and case["NF"] * (1 + case["automask"]) > 1:
        assert unjudged <= MC.MAX_UNJUDGED, unjudged
    assert 0.1 <= float(t["color"].min()) and float(t["color"].max()) <= 0.9001
    for which, (m, g64) in maps.items():
        assert int(m.max()) < case["NF"] * (1 + case["automask"]) and bool(g64.isfinite().all())
        assert not bool((g64 * (~MC.selected_near(case, m)).double()).any()), which      # zero wherever no window centre nearby selected the frame
        if which == "identity":
            assert not bool(g64.any())


def test_restated_sampler_equals_grid_sample():
    """`sample_border` (the form the defects are seeded in) with nothing seeded: torch's values and gradients."""
    run = ("ragged-2blk", 0, "none")
    case = MC.VS_BY_ID[run[0]]
    t, _, r64 = _vs(run)
    grid = r64["sample"][1, 1].clone().requires_grad_(True)
    src = t["src"].double()
    want = F.grid_sample(src[1], grid, padding_mode="border", align_corners=True)
    (gw,) = torch.autograd.grad((want * t["gcolor"][1, 1].double()).sum(), grid)
    got = MC.sample_border(src, 1, grid)
    (gg,) = torch.autograd.grad((got * t["gcolor"][1, 1].double()).sum(), grid)
    assert float((got - want).detach().abs().max()) <= 1e-14 and float((gg - gw).abs().max()) <= 1e-12 * float(gw.abs().max())


def test_restated_gather_and_patch_ssim_equal_autograd():
    """The stage-B restatement (up_matrix) and the patch form of the SSIM backward, with nothing dropped, against autograd."""
    g = torch.Generator().manual_seed(5)
    gu = torch.randn(2, 3, 8, 24, generator=g, dtype=torch.float64)
    low = torch.zeros(2, 3, 2, 6, dtype=torch.float64, requires_grad=True)
    (want,) = torch.autograd.grad((F.interpolate(low, (8, 24), mode="bilinear", align_corners=False) * gu).sum(), low)
    got = torch.einsum("iy,bcyx,jx->bcij", MC.up_matrix(2, 8), gu, MC.up_matrix(6, 24))
    assert float((got - want).abs().max()) <= 1e-13
    assert MC._reflect_index(2).tolist() == [1, 0, 1, 0] and MC._reflect_index(3).tolist() == [1, 0, 1, 2, 1]


# ---- rho32: the fp32 torch composition sets the scale of every bar ----------------------------------------------------------------------
_RHO = {}


def _rho_vs(run):
    if run not in _RHO:
        t, _, r64 = _vs(run)
        r32 = MC.vs_reference(t, MC.VS_BY_ID[run[0]], run[1], dtype=torch.float32)
        _RHO[run] = {n: MC.judge(n, r32[n], r64[n], A=r64["A_gT"] if n == "gT" else None, kappa=1.0)[0] for n in MC.vs_outputs(run[1])}
    return _RHO[run]


def _rho_ph(cid):
    if cid not in _RHO:
        case = MC.PH_BY_ID[cid]
        t, f64, maps = _ph(cid)
        f32 = MC.ph_forward(t, case, dtype=torch.float32)
        rho = dict(photo_value=MC.judge("photo_value", f32["values"].transpose(1, 2), f64["values"].transpose(1, 2), kappa=1.0)[0],
                   p_photo=MC.judge("p_photo", f32["p_photo"], f64["p_photo"], A=f64["A"], kappa=1.0)[0])
        rho["grad_color"] = max(MC.judge("grad_color", MC.ph_backward(t, case, m, dtype=torch.float32), g64, kappa=1.0)[0]
                                for m, g64 in maps.values())
        _RHO[cid] = rho
    return _RHO[cid]


@pytest.mark.parametrize("run", MC.VS_RUNS, ids=MC.vs_run_id)
def test_fp32_torch_stays_under_rho32_view_synthesis(run):
    rho = _rho_vs(run)
    print(MC.vs_run_id(run), {n: round(v, 2) for n, v in rho.items()})
    for n, v in rho.items():
        assert v <= MC.RHO32[n] * (0.5 if run[0] == "min2x2" else 1.0), (n, v)     # the smallest case sets no constant
    if run[0] == "min2x2":
        _, cond, _ = _vs(run)
        assert cond["unclipped"] > 0 and cond["fragile"] == 0, cond


@pytest.mark.parametrize("cid", [c["id"] for c in MC.PH_CASES])
def test_fp32_torch_stays_under_rho32_photometric(cid):
    rho = _rho_ph(cid)
    print(cid, {n: round(v, 2) for n, v in rho.items()})
    for n, v in rho.items():
        assert v <= MC.RHO32[n], (n, v)


def test_rho32_is_the_measured_maximum():
    """RHO32 is the measurement rounded up, no loose cap: at most twice the largest the table gives; kappa = max(2 rho32, 8)."""
    worst = {}
    for rho in [_rho_vs(r) for r in MC.VS_RUNS] + [_rho_ph(c["id"]) for c in MC.PH_CASES]:
        for n, v in rho.items():
            worst[n] = max(worst.get(n, 0.0), v)
    print("largest rho32 per output kind:", {n: round(v, 3) for n, v in worst.items()})
    assert set(worst) == set(MC.RHO32)
    for n, v in worst.items():
        assert v <= MC.RHO32[n] <= 2.0 * v, (n, v, MC.RHO32[n])
        assert MC.KAPPA[n] == max(2.0 * MC.RHO32[n], 8.0)


# ---- the defects --------------------------------------------------------------------------------------------------------------------
VS_D = [(d, run) for d, (runs, _) in MC.VS_DEFECTS.items() for run in runs]
PH_D = [(d, cid) for d, (cids, _) in MC.PH_DEFECTS.items() for cid in cids]


@pytest.mark.parametrize("defect,run", VS_D, ids=[f"{d}-{MC.vs_run_id(r)}" for d, r in VS_D])
def test_bars_see_the_view_synthesis_defect(defect, run):
    t, _, r64 = _vs(run)
    bad = MC.vs_reference(t, MC.VS_BY_ID[run[0]], run[1], defect=defect)
    seen = {n: MC.judge(n, bad[n], r64[n], A=r64["A_gT"] if n == "gT" else None)[0] for n in MC.vs_outputs(run[1])}
    print(defect, MC.vs_run_id(run), "largest error in units of the bar:", {n: round(v, 2) for n, v in seen.items()})
    for n in MC.VS_DEFECTS[defect][1]:
        assert seen[n] > 1.0, (defect, run, n, seen)


@pytest.mark.parametrize("defect,cid", PH_D, ids=[f"{d}-{c}" for d, c in PH_D])
def test_bars_see_the_photometric_defect(defect, cid):
    case = MC.PH_BY_ID[cid]
    t, f64, maps = _ph(cid)
    bad = MC.ph_forward(t, case, defect=defect)
    judged = MC.judged_pixels(f64) if case["special"] not in ("tie_warped", "tie_identity") else torch.ones_like(f64["argmin"], dtype=torch.bool)
    seen = dict(p_photo=MC.judge("p_photo", bad["p_photo"], f64["p_photo"], A=f64["A"])[0],
                argmin=float(((bad["argmin"] != f64["argmin"]) & judged).sum()))
    m, g64 = maps["reference"]
    seen["grad_color"] = MC.judge("grad_color", MC.ph_backward(t, case, m, defect=defect), g64)[0]
    print(defect, cid, "largest error in units of the bar (argmin: judged pixels that differ):", {n: round(v, 2) for n, v in seen.items()})
    for n in MC.PH_DEFECTS[defect][1]:
        assert (seen[n] > 0 if n == "argmin" else seen[n] > 1.0), (defect, cid, n, seen)
