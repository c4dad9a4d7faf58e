"""The cases, bars and defects of tests/attn_tiled_cases.py, checked without a GPU: the table against what each case claims to reach, the
restated tile sizes against the library, the emulation inside the bar with rho <= RHO_EMU (which fixes kappa), RHO_EMU against the measured
maximum, and the three defects the bars must see."""
import pytest
import torch

import attn_tiled_cases as AC
import mha_cases as MC

_REF, _FIGS = {}, {}


def _ref(case):
    if case["id"] not in _REF:
        t = AC.inputs(case)
        _REF[case["id"]] = (t,) + MC.reference(t, case, AC.weights(case))
    return _REF[case["id"]]


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    _REF.clear()
    _FIGS.clear()


def test_tile_sizes_are_the_library_s():
    from uenc import capi
    assert capi.lib.uenc_attn_tiled_tile(0) == AC.TQ and capi.lib.uenc_attn_tiled_tile(1) == AC.TK
    assert capi.lib.uenc_attn_tiled_tile(2) == -1


def test_case_table_reaches_what_it_names():
    ids = [c["id"] for c in AC.CASES]
    assert len(set(ids)) == len(ids)
    for c in AC.CASES:
        assert c["B"] * c["H"] * c["Lq"] * c["S"] <= MC.MAX_SCORES, c["id"]
        assert not c["masked"]
    edge = lambda n: {n - 1, n, n + 1, 2 * n + 1}
    assert {c["Lq"] for c in AC.CASES} >= edge(AC.TQ) | {1, 28, 70, 1000}
    assert {c["S"] for c in AC.CASES} >= edge(AC.TK) | {1, 28, 33, 1000}
    C = AC.BY_ID
    assert (C["one"]["Lq"], C["one"]["S"]) == (1, 1) and (C["q70-s33"]["Lq"], C["q70-s33"]["S"]) == (70, 33)
    assert (C["res5-28"]["Lq"], C["res5-28"]["S"], C["res5-28"]["H"]) == (28, 28, 4)
    assert (C["q1000"]["B"], C["q1000"]["H"], C["q1000"]["Lq"], C["q1000"]["S"]) == (1, 2, 1000, 1000)
    assert all(C["q1000"]["Lq"] > lq for _, lq in MC.BWD_REJECT_LQ)                  # past what uenc_mha_bwd accepts
    assert {c["H"] for c in AC.CASES} >= {1, 2, 3, 8} and max(c["B"] for c in AC.CASES) == 3
    D = [c for c in AC.CASES if c["p"] > 0]
    assert {c["p"] for c in D} == {0.1} and {c["seed_mode"] for c in D} == {"host", "slot"}
    assert all(c["Lq"] % AC.TQ and c["S"] % AC.TK for c in D)                        # dropout meets a ragged tile and a ragged block
    assert all(set(v) <= set(C) for v in AC.DEFECT_CASES.values()) and set(AC.DEFECT_CASES) == set(AC.DEFECT_REACH)


def _figs(case):
    """Per output (rho, worst share of the bar) of the emulation, and its lse error: computed once per case."""
    if case["id"] not in _FIGS:
        t, r64, A = _ref(case)
        emu = MC.emulate(t, case, AC.weights(case))
        f = {n: (MC.rho(n, emu[n], r64[n], A[n]), float(((emu[n] - r64[n]).abs() / AC.bar(n, r64[n], A[n])).max())) for n in AC.OUTPUTS}
        f["lse"] = float((emu["lse"] - r64["lse"]).abs().max())
        _FIGS[case["id"]] = f
    return _FIGS[case["id"]]


@pytest.mark.parametrize("case", AC.CASES, ids=lambda c: c["id"])
def test_emulation_stays_inside_the_bar(case):
    _, r64, A = _ref(case)
    figs = _figs(case)
    print(case["id"], "rho, worst share of the bar:", {n: (round(figs[n][0], 3), round(figs[n][1], 3)) for n in AC.OUTPUTS})
    for n in AC.OUTPUTS:
        assert bool((A[n] >= 0).all()) and bool(r64[n].isfinite().all())
        assert figs[n][0] <= AC.RHO_EMU[n], (case["id"], n, figs)
        assert figs[n][1] <= 1.0, (case["id"], n, figs)
    assert figs["lse"] <= 1e-12 * max(1.0, float(r64["lse"].abs().max()))


def test_rho_emu_is_the_measured_maximum():
    """RHO_EMU is the measurement rounded up, not a loose cap: at most 10 % above the largest rho the table gives."""
    worst = {n: max((_figs(c)[n][0], c["id"]) for c in AC.CASES) for n in AC.OUTPUTS}
    print("largest rho per output:", {n: (round(v, 3), i) for n, (v, i) in worst.items()}, "kappa:", AC.KAPPA)
    for n in AC.OUTPUTS:
        assert worst[n][0] <= AC.RHO_EMU[n] <= 1.1 * worst[n][0], (n, worst[n], AC.RHO_EMU[n])
        assert AC.KAPPA[n] == 2.0 * AC.RHO_EMU[n]


DEFECTS = [(d, cid) for d, cids in AC.DEFECT_CASES.items() for cid in cids]


@pytest.mark.parametrize("defect,cid", DEFECTS, ids=[f"{d}-{c}" for d, c in DEFECTS])
def test_bars_see_the_defect(defect, cid):
    case = AC.BY_ID[cid]
    t, r64, A = _ref(case)
    bad = AC.defective(defect, t, case)
    seen = {}
    for n in AC.OUTPUTS:
        err = (bad[n] - r64[n]).abs()
        assert bool(err.isfinite().all())
        seen[n] = float((err / AC.bar(n, r64[n], A[n])).max())
    seen["lse"] = float((bad["lse"] - r64["lse"]).abs().max()) / MC.lse_bar(r64["lse"], MC.lse_fp32(t, case))[1]
    print(defect, cid, "largest error in units of the bar:", {n: round(v, 2) for n, v in seen.items()})
    for n in AC.DEFECT_REACH[defect]:
        assert seen[n] > 1.0, (defect, cid, n, seen)
    for n in set(AC.OUTPUTS + ("lse",)) - set(AC.DEFECT_REACH[defect]):
        assert seen[n] == 0.0, (defect, cid, n, seen)                          # and the defect is the only difference
