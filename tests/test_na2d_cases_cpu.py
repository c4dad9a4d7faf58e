"""The cases, references and bars of tests/na2d_cases.py, checked without a GPU: the restated planner against what each case claims to
reach, r64 against the oracle's two forms and against the closed forms over explicit maps, the emulation inside its bars with
rho <= RHO_EMU (which fixes kappa), emu32 with rho32 <= RHO32 (which fixes gamma), the float reciprocal division of the tile walk, and
the defects the bars must see."""
import numpy as np
import pytest
import torch

import na2d_cases as NC

_REF = {}


def _ref(case):
    """(inputs, r64, closed forms, A, emulation, emu32) of one case, on the heads the CPU measurement uses (all of them but in the nt*
    cases: first, last, one in between -- heads are independent): computed once per module and left unchanged."""
    if case["id"] not in _REF:
        t = NC.inputs(case)
        heads = NC.EMU_HEADS.get(case["id"])
        cf, A = NC.neigh(t, case, heads=heads)
        _REF[case["id"]] = (t, NC.reference(t, case, heads=heads), cf, A, NC.emulate(t, case, heads=heads),
                            NC.reference(t, case, torch.float32, heads=heads))
    return _REF[case["id"]]


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    _REF.clear()
    _FIGS.clear()


def test_case_table_is_well_formed():
    ids = [c["id"] for c in NC.CASES]
    assert len(set(ids)) == len(ids)
    for c in NC.CASES:
        B, H, W, nH, K, d = NC.dims(c)
        assert K in (3, 5, 7, 9, 11, 13) and H >= K * d and W >= K * d, c["id"]       # na2d_check
        assert NC.n_scores(c) <= NC.MAX_SCORES and B * H * W * 96 * nH <= NC.MAX_QKV, c["id"]
        assert NC.route(c) == ("mfma" if K <= 7 else "valu")                          # no case near the 2^31 extent (module docstring)
    assert {c["K"] for c in NC.CASES} == {3, 5, 7, 9, 11, 13}
    assert all(set(v) <= set(NC.BY_ID) for v in NC.DEFECT_CASES.values()) and set(NC.DEFECT_CASES) == set(NC.DEFECT_REACH)
    assert [c["id"] for c in NC.F32_CASES] == ["min3", "min7", "min5-d3", "short7", "ragged5", "kvmax7", "ncb2", "notok3", "tail65", "valu9", "valu11",
                                               "valu13-halo", "valu13-w", "no-rpb", "no-rpb9"]
    assert NC.BY_ID["no-rpb"]["rpb"] is False and NC.BY_ID["no-rpb9"]["rpb"] is False and NC.inputs(NC.BY_ID["no-rpb"])["rpb"] is None


# id -> what the case reaches, every field of `reach` spelt out (hh_max, hw_max, ncb: the per-key MFMA kernel's, 0 on the VALU route; halo: the
# largest halo of the VALU tiled kernels; notok_walks: the walks that hold a !ok tile in some residue class; notok_prefetched: such a
# tile is not the first of its walk, so it is reached as the prefetched tile)
REACHES = {
    "min3": dict(route="mfma", nt=1, walks=[[0]], crosses_row=False, notok_walks=[], notok_prefetched=False, class_len_y=[3], class_len_x=[3], hh_max=3, hw_max=3, ncb=1, grid=(1, 1, 1)),
    "min7": dict(route="mfma", nt=1, walks=[[0]], crosses_row=False, notok_walks=[], notok_prefetched=False, class_len_y=[7], class_len_x=[7], hh_max=7, hw_max=7, ncb=1, grid=(1, 1, 1)),
    "min5-d3": dict(route="mfma", nt=1, walks=[[0]], crosses_row=False, notok_walks=[], notok_prefetched=False, class_len_y=[5, 5, 5], class_len_x=[6, 6, 5], hh_max=5, hw_max=6, ncb=1, grid=(1, 9, 2)),
    "short7": dict(route="mfma", nt=1, walks=[[0], [1]], crosses_row=False, notok_walks=[], notok_prefetched=False, class_len_y=[13], class_len_x=[14], hh_max=13, hw_max=14, ncb=1, grid=(2, 1, 2)),
    "ragged5": dict(route="mfma", nt=1, walks=[[0], [1], [2], [3]], crosses_row=False, notok_walks=[], notok_prefetched=False, class_len_y=[11, 10], class_len_x=[23, 22], hh_max=11, hw_max=18, ncb=1, grid=(4, 4, 3)),
    "kvmax7": dict(route="mfma", nt=1, walks=[[0], [1], [2], [3], [4], [5], [6], [7], [8]], crosses_row=False, notok_walks=[], notok_prefetched=False, class_len_y=[22], class_len_x=[38], hh_max=17, hw_max=25, ncb=2, grid=(9, 1, 4)),
    "ncb2": dict(route="mfma", nt=1, walks=[[0], [1], [2], [3]], crosses_row=False, notok_walks=[], notok_prefetched=False, class_len_y=[9], class_len_x=[22], hh_max=9, hw_max=22, ncb=2, grid=(4, 1, 1)),
    "notok3": dict(route="mfma", nt=1, walks=[[0], [1], [2]], crosses_row=False, notok_walks=[[2]], notok_prefetched=False, class_len_y=[4, 4, 4, 4], class_len_x=[33, 33, 32, 32], hh_max=4, hw_max=18, ncb=1, grid=(3, 16, 1)),
    "tail65": dict(route="mfma", nt=1, walks=[[0], [1], [2], [3], [4]], crosses_row=False, notok_walks=[], notok_prefetched=False, class_len_y=[8], class_len_x=[65], hh_max=8, hw_max=18, ncb=1, grid=(5, 1, 1)),
    "nt2-tail": dict(route="mfma", nt=2, walks=[[0, 1], [2]], crosses_row=False, notok_walks=[[2]], notok_prefetched=False, class_len_y=[3, 3, 3, 3], class_len_x=[33, 32, 32, 32], hh_max=3, hw_max=18, ncb=1, grid=(2, 16, 64)),
    "nt3-notok": dict(route="mfma", nt=3, walks=[[0, 1, 2]], crosses_row=False, notok_walks=[[0, 1, 2]], notok_prefetched=True, class_len_y=[3, 3, 3, 3], class_len_x=[33, 32, 32, 32], hh_max=3, hw_max=18, ncb=1, grid=(1, 16, 96)),
    "nt2-rows": dict(route="mfma", nt=2, walks=[[0, 1], [2, 3], [4, 5]], crosses_row=True, notok_walks=[[2, 3], [4, 5]], notok_prefetched=True, class_len_y=[9, 9, 9, 9], class_len_x=[33, 32, 32, 32], hh_max=9, hw_max=20, ncb=1, grid=(3, 16, 32)),
    "nt8": dict(route="mfma", nt=8, walks=[[0, 1, 2, 3, 4, 5, 6, 7]], crosses_row=False, notok_walks=[], notok_prefetched=False, class_len_y=[3, 3, 3, 3], class_len_x=[113, 113, 113, 113], hh_max=3, hw_max=18, ncb=1, grid=(1, 16, 96)),
    "valu9": dict(route="valu", nt=0, walks=[], crosses_row=False, notok_walks=[], notok_prefetched=False, class_len_y=[10, 9], class_len_x=[19, 18], hh_max=0, hw_max=0, ncb=0, grid=(4, 4, 1), halo=(10, 19)),
    "valu11": dict(route="valu", nt=0, walks=[], crosses_row=False, notok_walks=[], notok_prefetched=False, class_len_y=[12], class_len_x=[50], hh_max=0, hw_max=0, ncb=0, grid=(4, 2, 2), halo=(12, 26)),
    "valu13-halo": dict(route="valu", nt=0, walks=[], crosses_row=False, notok_walks=[], notok_prefetched=False, class_len_y=[24], class_len_x=[40], hh_max=0, hw_max=0, ncb=0, grid=(3, 3, 1), halo=(20, 28)),
    "valu13-w": dict(route="valu", nt=0, walks=[], crosses_row=False, notok_walks=[], notok_prefetched=False, class_len_y=[13], class_len_x=[130], hh_max=0, hw_max=0, ncb=0, grid=(9, 2, 4), halo=(13, 28)),
    "no-rpb": dict(route="mfma", nt=1, walks=[[0], [1]], crosses_row=False, notok_walks=[[1]], notok_prefetched=False, class_len_y=[8, 8], class_len_x=[17, 16], hh_max=8, hw_max=17, ncb=1, grid=(2, 4, 2)),
    "no-rpb9": dict(route="valu", nt=0, walks=[], crosses_row=False, notok_walks=[], notok_prefetched=False, class_len_y=[10, 9], class_len_x=[19, 18], hh_max=0, hw_max=0, ncb=0, grid=(4, 4, 2), halo=(10, 19)),
}


@pytest.mark.parametrize("case", NC.CASES, ids=lambda c: c["id"])
def test_case_reaches_what_the_table_names(case):
    r = NC.reach(case)
    print(case["id"], r)
    assert set(REACHES[case["id"]]) >= {"route", "nt", "walks", "crosses_row", "notok_walks", "notok_prefetched", "class_len_y", "class_len_x", "hh_max",
                                        "hw_max", "ncb"}
    for k, v in REACHES[case["id"]].items():
        assert r[k] == v, (case["id"], k, r[k], v)


def test_the_walks_in_detail():
    C = NC.BY_ID
    tiles = lambda c: NC.plan(c["B"], c["H"], c["W"], c["nH"], c["d"])["per_class"] * c["d"] ** 2 * c["B"] * c["nH"]
    assert [tiles(C[i]) for i in NC.NT_CASES] == [3072, 4608, 3072, 12288]
    assert max(tiles(c) for c in NC.CASES if c["id"] not in NC.NT_CASES) < 1536 * 2        # everything else: nt == 1
    # the largest parametrisation of tests/test_dinat_gpu.py::test_na2d_kernels_vs_oracle: 216 tiles
    assert NC.plan(1, 48, 200, 2, 6)["nt"] == 1 and NC.plan(1, 48, 200, 2, 6)["per_class"] * 36 * 1 * 2 == 216 < 1536
    # B = 1 halves the tile count: another nt and another chunking in every nt* case
    for i, nt2, nt1 in (("nt2-tail", 2, 1), ("nt3-notok", 3, 1), ("nt2-rows", 2, 1), ("nt8", 8, 4)):
        c = C[i]
        assert NC.tiles_per_group(2, c["H"], c["W"], c["nH"], c["K"], c["d"]) == nt2 and NC.tiles_per_group(1, c["H"], c["W"], c["nH"], c["K"], c["d"]) == nt1
    # nt2-tail: the clipped last chunk is !ok in the three classes with 32 columns
    g = lambda Lx: NC.tile_q(2, 3, 3, Lx, 3)
    assert g(33)["ok"] and not g(32)["ok"]
    # nt2-rows: between tiles 0 and 1 the wx = 0 waves change bcol0 (6 at the left border, 3 inside), the wx = 1 waves keep theirs
    first = lambda pa, L, K: NC._clamp(pa - K // 2, 0, L - K) - pa + K - 1
    assert (first(0, 33, 7), first(16, 33, 7)) == (6, 3) and first(8, 33, 7) == first(24, 33, 7) == 3
    # ncb2: keys 8 .. 15 of 22 see the queries 5 .. 21; the second tile row has one position, so only the wy = 0 waves are active there
    assert (NC._inv_start(8, 7), NC._inv_end(15, 22, 7)) == (5, 22) and NC.tile_q(2, 2, 9, 22, 7)["py0"] == 8
    # kvmax7: the tile whose last key is the first of the clamped border band
    assert NC._inv_end(15, 22, 7) - NC._inv_start(8, 7) == 17 and NC._inv_end(31, 38, 7) - NC._inv_start(16, 7) == 25
    # valu13-halo: an interior tile row / column whose windows are clamped on neither side exists (uniform waves), and border ones
    assert NC.tile_q(4, 3, 24, 40, 13)["hh"] == 20 and NC.tile_q(4, 3, 24, 40, 13)["hw"] == 28
    # ... and both drpb paths of na2d_bwd_q_tiled_kernel<13>: the 16 pixels of a wave share the bias column in the middle tile column
    # (`uniform`), not in the two at the borders
    pbx = lambda px: NC._clamp(px - 6, 0, 40 - 13) - px + 12
    assert len({pbx(px) for px in range(16, 32)}) == 1 and len({pbx(px) for px in range(0, 16)}) > 1 and len({pbx(px) for px in range(32, 40)}) > 1
    assert -(-C["valu13-w"]["W"] // 64) == 3 and C["valu13-w"]["W"] % 64 and C["valu11"]["W"] < 64
    assert NC.drpb_adds(C["nt2-rows"]) == 3 * 16 * 2 and NC.drpb_adds(C["valu13-w"]) == 9 * 2 * 2 and NC.drpb_adds(C["nt8"]) == 16 * 2


def test_library_reports_the_restated_planner():
    """uenc_na2d_tiles_per_group is host code only (include/uenc_ext.h, csrc/ext/na2d_plan.hip; it calls na2d_mfma_plan, the function both launchers plan by):
    nt on the MFMA route, 0 where the VALU kernels run, < 0 for what uenc_na2d_fwd refuses -- against the restatement, for every case at
    its own batch size and at B = 1, and for a sweep around the thresholds of the heuristic."""
    from uenc import capi
    f = capi.lib.uenc_na2d_tiles_per_group
    assert "uenc_na2d_tiles_per_group" in capi.EXT_FUNCTIONS and "uenc_na2d_tiles_per_group" not in capi.FUNCTIONS
    for c in NC.CASES:
        B, H, W, nH, K, d = NC.dims(c)
        for b in (B, 1):
            assert f(b, H, W, nH, K, d) == NC.tiles_per_group(b, H, W, nH, K, d) == (NC.reach(dict(c, B=b))["nt"]), (c["id"], b)
    for B, H, W, nH, K, d in [(1, 8, 16, 1535, 3, 1), (1, 8, 16, 1536, 3, 1), (1, 8, 16, 3071, 3, 1), (1, 8, 17, 1536, 3, 1), (2, 160, 160, 6, 7, 1),
                              (4, 160, 160, 12, 7, 2), (8, 80, 80, 24, 7, 1), (16, 40, 40, 48, 7, 1), (1, 24, 40, 1, 13, 1), (1, 7, 7, 1, 7, 1)]:
        assert f(B, H, W, nH, K, d) == NC.tiles_per_group(B, H, W, nH, K, d), (B, H, W, nH, K, d)
    assert f(1, 8, 16, 1536, 3, 1) == 1 and f(1, 8, 17, 1536, 3, 1) == 2 and f(1, 24, 40, 1, 13, 1) == 0      # one tile per class caps nt
    assert f(1, 6, 20, 1, 7, 1) < 0 and f(1, 20, 20, 1, 4, 1) < 0 and f(0, 20, 20, 1, 3, 1) < 0                # as uenc_na2d_fwd refuses them


@pytest.mark.parametrize("length,K,d", [(3, 3, 1), (7, 7, 1), (13, 7, 1), (14, 7, 1), (15, 5, 3), (17, 5, 3), (21, 5, 2), (45, 5, 2), (129, 3, 4),
                                        (129, 7, 4), (36, 7, 4), (452, 3, 4), (19, 9, 2), (37, 9, 2), (50, 11, 1), (24, 13, 1), (130, 13, 1), (33, 7, 2)])
def test_closed_form_equals_nattens_formulas(length, K, d):
    """The closed form the defects are built on, without a defect, against NATTEN's literal formulas; no neighbour leaves the axis."""
    nb, pb = NC.natten_axis(length, K, d)
    cb, cp = NC.closed_axis(length, K, d)
    assert torch.equal(nb, cb) and torch.equal(pb, cp)
    assert int(nb.min()) >= 0 and int(nb.max()) < length and int(pb.min()) >= 0 and int(pb.max()) < 2 * K - 1


def test_fdiv_is_exact_where_the_kernels_use_it():
    """`(int)(((float)a + 0.5f) * inv_b)` equals a // b at the only places a floor can flip, a = q b - 1 and a = q b: for every
    b = tiles_x with tiles_x tiles_y < 2^18 (above the 175 k tiles per class that H W 3C < 2^31 admits), and for every b = hw_max <= 25 of
    the per-key kernel's staging with a < 17 * 25 + 32."""
    for b in range(1, 2 ** 18):
        q = np.arange(1, 2 ** 18 // b + 1, dtype=np.int64)
        a = np.concatenate([q * b - 1, q * b])
        a = a[a < 2 ** 18]
        assert np.array_equal(NC.fdiv(a, b), (a // b).astype(np.int32)), b
    for b in range(1, 26):
        a = np.arange(0, 17 * 25 + 32)
        assert np.array_equal(NC.fdiv(a, b), (a // b).astype(np.int32)), b


@pytest.mark.parametrize("cid", ["min3", "min5-d3", "short7", "ragged5", "valu9", "no-rpb"])
def test_reference_equals_the_oracle(cid):
    """r64 against oracle.dinat_ref.na2d (gather form) and, on the smallest maps, na2d_dense (explicit mask), in float64 with their own autograd."""
    from oracle import dinat_ref as D
    case = NC.BY_ID[cid]
    t, r64 = _ref(case)[:2]
    B, H, W, nH, K, d = NC.dims(case)
    forms = (D.na2d, D.na2d_dense) if H * W <= 300 else (D.na2d,)
    for form in forms:
        x = t["qkv"].double().permute(3, 0, 4, 1, 2, 5).contiguous().requires_grad_(True)
        r = (torch.zeros(nH, 2 * K - 1, 2 * K - 1) if t["rpb"] is None else t["rpb"]).double().requires_grad_(True)
        before = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)                                       # na2d_dense builds its mask in the default dtype
        try:
            out = form(x[0] * NC.SCALE, x[1], x[2], r, K, d).permute(0, 2, 3, 1, 4)
        finally:
            torch.set_default_dtype(before)
        grads = torch.autograd.grad(out, [x, r], t["dout"].double())
        want = dict(out=out.detach(), dqkv=grads[0].permute(1, 3, 4, 0, 2, 5), drpb=grads[1])
        for n in NC.OUTPUTS:
            assert float((r64[n] - want[n]).abs().max()) <= 1e-12 * max(1.0, float(want[n].abs().max())), (form.__name__, n)


@pytest.mark.parametrize("case", NC.CASES, ids=lambda c: c["id"])
def test_closed_forms_equal_autograd(case):
    """The closed forms over explicit (query, slot) maps that the emulation and the defects are built on, unrounded, against r64; lse too."""
    _, r64, cf, A, _, _ = _ref(case)
    for n in NC.OUTPUTS + ("lse",):
        assert cf[n].shape == r64[n].shape
        assert float((cf[n] - r64[n]).abs().max()) <= 1e-12 * max(1.0, float(r64[n].abs().max())), n
    for n in NC.OUTPUTS:
        assert A[n].shape == r64[n].shape and bool((A[n] >= 0).all()) and bool((A[n] >= r64[n].abs() * (1 - 1e-9)).all()), n


_FIGS = {}


def _kappa(case, n, table=None):
    return (NC.KAPPA if table is None else table)[NC.route(case)][n]


def _figs(case):
    if case["id"] not in _FIGS:
        _, r64, _, A, emu, e32 = _ref(case)
        _FIGS[case["id"]] = dict(
            rho={n: NC.rho(n, emu[n], r64[n], A[n]) for n in NC.OUTPUTS}, rho32={n: NC.rho32(n, e32[n], r64[n], A[n]) for n in NC.OUTPUTS},
            share={n: float(((emu[n] - r64[n]).abs() / NC.bar(n, r64[n], A[n], _kappa(case, n))).max()) for n in NC.OUTPUTS},
            share32={n: float(((e32[n].double() - r64[n]).abs() / NC.bar32(n, r64[n], A[n])).max()) for n in NC.OUTPUTS},
            lse=float((emu["lse"] - r64["lse"]).abs().max()))
    return _FIGS[case["id"]]


@pytest.mark.parametrize("case", NC.CASES, ids=lambda c: c["id"])
def test_emulations_stay_inside_the_bars(case):
    r64 = _ref(case)[1]
    f = _figs(case)
    print(case["id"], NC.route(case), {k: {n: round(v, 3) for n, v in f[k].items()} for k in ("rho", "share", "rho32", "share32")})
    for n in NC.OUTPUTS:
        assert bool(r64[n].isfinite().all())
        assert f["rho"][n] <= NC.RHO_EMU[NC.route(case)][n] and f["share"][n] <= 1.0, (case["id"], n, f)
        assert f["rho32"][n] <= NC.RHO32[n] and f["share32"][n] <= 1.0, (case["id"], n, f)
    assert f["lse"] <= 1e-12 * max(1.0, float(r64["lse"].abs().max()))            # no rounding point touches the statistics


def test_rho_is_the_measured_maximum():
    """RHO_EMU (per route) and RHO32 are the measurements rounded up, not loose caps: at most 10 % above the largest ratio the table gives
    (two decimals: 0.01 above it where the ratio itself is below 0.1); gamma 2^-24 stays below 2^-14 -- beyond that the fp32 bar would
    no longer be an fp32-level bar and its margin would have to be derived again, not widened."""
    for rt in ("mfma", "valu"):
        cases = [c for c in NC.CASES if NC.route(c) == rt]
        worst = {n: max((_figs(c)["rho"][n], c["id"]) for c in cases) for n in NC.OUTPUTS}
        print("largest rho", rt, worst, NC.KAPPA[rt])
        for n in NC.OUTPUTS:
            assert worst[n][0] <= NC.RHO_EMU[rt][n] <= max(1.1 * worst[n][0], worst[n][0] + 0.01), (rt, n, worst[n], NC.RHO_EMU[rt][n])
            assert NC.KAPPA[rt][n] == 2.0 * NC.RHO_EMU[rt][n]
    worst = {n: max((_figs(c)["rho32"][n], c["id"]) for c in NC.CASES) for n in NC.OUTPUTS}
    print("largest rho32", worst, NC.GAMMA)
    for n in NC.OUTPUTS:
        assert worst[n][0] <= NC.RHO32[n] <= 1.1 * worst[n][0], (n, worst[n], NC.RHO32[n])
        assert NC.GAMMA[n] == 8.0 * NC.RHO32[n]
    assert max(NC.GAMMA.values()) * NC.U24 < 2.0 ** -14


DEFECTS = [(d, cid) for d, cids in NC.DEFECT_CASES.items() for cid in cids]
_PARTS = ("out", "lse", "dq", "dk", "dv", "drpb")


def _names(reach):
    """"dqkv" stands for its three slices."""
    return [p for n in reach for p in (("dq", "dk", "dv") if n == "dqkv" else (n,))]


@pytest.mark.parametrize("defect,cid", DEFECTS, ids=[f"{d}-{c}" for d, c in DEFECTS])
def test_bars_see_the_defect(defect, cid):
    """The defect applied to the emulation: every output it must reach leaves its bar, every output it cannot reach keeps its bits.  The
    defect with an empty reach is the one tests/na2d_cases.py documents as within the bar: it must stay inside it here, so that the
    documentation cannot go stale unnoticed."""
    case = NC.BY_ID[cid]
    t, r64, _, A, emu, e32 = _ref(case)
    bad = NC.emulate(t, case, defect, heads=NC.EMU_HEADS.get(cid))
    seen = {}
    for p in _PARTS:
        err = (NC.part(bad, p) - NC.part(r64, p)).abs()
        assert bool(err.isfinite().all())
        if p == "lse":
            seen[p] = float(err.max()) / NC.lse_bar(r64["lse"], e32["lse"])[1]
        else:
            n = "dqkv" if p in ("dq", "dk", "dv") else p
            seen[p] = float((err / NC.part(dict(r64, **{n: NC.bar(n, r64[n], A[n], _kappa(case, n))}), p)).max())
    print(defect, cid, "largest error in units of the bar:", {n: round(v, 2) for n, v in seen.items()})
    for p in _names(NC.DEFECT_REACH[defect]):
        assert seen[p] > 1.0, (defect, cid, p, seen)
    for p in _names(NC.DEFECT_UNTOUCHED.get(defect, ())):
        assert torch.equal(NC.part(bad, p), NC.part(emu, p)), (defect, cid, p)
    if not NC.DEFECT_REACH[defect]:
        assert all(v <= 1.0 for v in seen.values()), (defect, cid, seen)
    if defect == "c_bias_ignores_clamp" and cid == "nt2-rows":
        # what tests/test_dinat_gpu.py::test_na2d_kernels_vs_oracle measures: the relative L2 error over the whole tensor, next to its bars
        rel = lambda a, b: float((a - b).norm() / b.norm())
        l2 = {p: rel(NC.part(bad, p), NC.part(r64, p)) for p in ("out", "dq", "dk", "dv", "drpb")}
        sound = {p: rel(NC.part(emu, p), NC.part(r64, p)) for p in ("out", "dq", "dk", "dv", "drpb")}
        print("relative L2 error with the defect:", {p: f"{v:.2e}" for p, v in l2.items()}, "without:", {p: f"{v:.2e}" for p, v in sound.items()},
              "-- the tensor-wide bars are 1e-2 (out) and 2e-2 (gradients)")
        # printed and recorded, not asserted: at K = 7 and d = 4 every class of this case is 9 positions tall, so almost every pixel is
        # a border pixel and the norm does see this defect here -- had the old test run at this size
        from conftest import record_parity
        record_parity("na2d_cpu/defect_c_bias_ignores_clamp/nt2-rows", bar_out=1e-2, bar_gradients=2e-2,
                      **{f"rel_l2_{p}_with_defect": v for p, v in l2.items()}, **{f"rel_l2_{p}_sound": v for p, v in sound.items()})
