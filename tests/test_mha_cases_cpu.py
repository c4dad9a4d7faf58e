"""The cases, references and bars of tests/mha_cases.py, checked without a GPU: the closed-form reference against autograd, the table
against what each case claims to reach, the emulation inside the bar with rho <= RHO_EMU (which fixes kappa), and the eight defects the
bars must see."""
import math

import pytest
import torch

import mha_cases as MC

_REF = {}


def _weights(case):
    if case["p"] == 0.0:
        return None
    from uenc.attention import keep_mask_reference
    keep = keep_mask_reference(case["B"], case["H"], case["Lq"], case["S"], case["p"], MC.DROP_SEED)
    return keep.double() / (1.0 - case["p"])


def _ref(case):
    if case["id"] not in _REF:
        t = MC.inputs(case)
        _REF[case["id"]] = (t,) + MC.reference(t, case, _weights(case))
    return _REF[case["id"]]


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    _REF.clear()
    _FIGS.clear()


def test_case_table_is_well_formed():
    ids = [c["id"] for c in MC.CASES]
    assert len(set(ids)) == len(ids)
    for c in MC.CASES:
        B, H, Lq, S = c["B"], c["H"], c["Lq"], c["S"]
        assert B * H * Lq * S <= MC.MAX_SCORES, c["id"]
        assert MC.splits(B, H, S)[0] == c["nsplit"], c["id"]
        slices = -(-Lq // MC.MQ)
        lds = slices * MC.MQ * 136 + 16384 + (64 * (slices * MC.MQ + 4) if c["masked"] else 0)
        assert lds <= 160 * 1024, c["id"]                                     # the backward accepts it
        if c["masked"]:
            m = MC.make_mask(c)
            assert bool((~m).any(-1).all()), c["id"]                          # no fully blocked row
            assert bool(m[0, 0, :-1].all()) and not bool(m[0, 0, -1])         # a row that sees only the last key
            if B * Lq > 8 and S >= 63:
                assert 0.5 < float(m.double().mean()) < 0.7
    for masked, Lq in MC.BWD_REJECT_LQ:                                       # one query more than the largest accepted, refused for LDS alone
        slices = -(-Lq // MC.MQ)
        assert slices * MC.MQ * 136 + 16384 + (64 * (slices * MC.MQ + 4) if masked else 0) > 160 * 1024
        assert any(c["Lq"] == Lq - 1 and c["masked"] == masked for c in MC.CASES)


def test_case_table_reaches_what_it_names():
    C, sp = MC.BY_ID, lambda c: MC.splits(c["B"], c["H"], c["S"])
    grid = lambda c: c["nsplit"] * c["B"] * c["H"]
    assert {c["H"] for c in MC.CASES} >= {1, 2, 3, 6, 8}
    for i in ("h1", "h3", "h2", "h6", "h8-tail", "dbuf"):                     # padded tail blocks, odd and even H
        assert grid(C[i]) % 16 != 0
    assert {C[i]["H"] % 2 for i in ("h1", "h3")} == {1} and C["h6"]["H"] == 6 and C["h8-tail"]["H"] == 8 and C["dbuf"]["H"] == 6
    assert {c["S"] for c in MC.CASES} >= {1, 3, 63, 64, 65, 127, 128, 129}
    for masked in (False, True):
        assert {c["Lq"] for c in MC.CASES if c["masked"] == masked and c["p"] == 0.0} >= {1, 15, 16, 17, 159, 160, 161}
    # a split that owns one key, with B H = 8
    for i in ("s65-2split", "s4097", "s4033-64split"):
        ns, per = sp(C[i])
        assert C[i]["B"] * C[i]["H"] == 8 and C[i]["S"] - (ns - 1) * per == 1
    assert sp(C["s65-2split"])[0] == 2 and sp(C["s4033-64split"]) == (64, 64)
    assert -(-C["s4097"]["S"] // MC.KB) > 64 and sp(C["s4097"])[1] == 128      # more blocks than the cap allows splits
    # one split over several blocks
    for i, nblk in (("bh768-s130", 3), ("bh768-s200", 4), ("drop-bh768", 3)):
        assert C[i]["B"] * C[i]["H"] == 768 and sp(C[i]) == (1, nblk * MC.KB) and -(-C[i]["S"] // MC.KB) == nblk
    # several blocks per split and several splits; masked with one slice (register staging) and with four (loop staging)
    assert sp(C["dbuf"]) == (17, 128) and C["dbuf"]["masked"] and C["dbuf"]["Lq"] <= MC.MQ
    assert sp(C["q481-m"]) == (33, 128) and C["q481-m"]["masked"] and -(-C["q481-m"]["Lq"] // MC.MQ) == 4
    assert 4 * MC.MQ * 136 + 16384 + 64 * (4 * MC.MQ + 4) > 64 * 1024            # the opt-in to more than 64 KB of LDS
    assert (C["q640-m"]["Lq"], C["q640-m"]["masked"], C["q960-u"]["Lq"], C["q960-u"]["masked"]) == (640, True, 960, False)
    # mask rows: S % 4 in {1, 2, 3}
    assert {c["S"] % 4 for c in MC.CASES if c["masked"]} >= {1, 2, 3}
    # rows blocked in a whole block / a whole split but visible elsewhere
    for i in ("h1", "q160-m", "dbuf", "s4097"):
        c = C[i]; m = MC.make_mask(c); ns, per = sp(c)
        assert bool(m[0, 2, :MC.KB].all()) and bool(m[0, 3, :per].all()) and bool(m[0, 4, (ns - 1) * per:].all())
    # dropout: both rates, masked and not, one split and many, a second slice
    D = [c for c in MC.CASES if c["p"] > 0]
    assert {c["p"] for c in D} == {0.1, 0.5} and {c["masked"] for c in D} == {False, True}
    assert {c["nsplit"] == 1 for c in D} == {False, True} and any(c["Lq"] == 161 for c in D)
    # the single-key rows the GPU test compares bit for bit
    assert len(MC.single_key_rows(C["s1"])) == 10 and (0, 0, C["h1"]["S"] - 1) in MC.single_key_rows(C["h1"])
    assert all(set(v) <= set(C) for v in MC.DEFECT_CASES.values()) and set(MC.DEFECT_CASES) == set(MC.DEFECT_REACH)


@pytest.mark.parametrize("cid", ["h3", "q17-m", "drop-3split-m"])
def test_reference_equals_autograd(cid):
    """The closed forms against float64 autograd through an independently written softmax attention, and lse against torch.logsumexp."""
    case = MC.BY_ID[cid]
    t, r64, _ = _ref(case)
    w = _weights(case)
    B, H = case["B"], case["H"]
    leaves = [t[n].double().requires_grad_(True) for n in ("q", "k", "v")]
    q, k, v = (a.view(B, -1, H, 32).transpose(1, 2) for a in leaves)
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) / math.sqrt(32.0)
    if t["mask"] is not None:
        s = s + torch.zeros_like(s).masked_fill(t["mask"][:, None], -math.inf)
    p = torch.softmax(s, -1)
    out = torch.einsum("bhqk,bhkd->bqhd", p if w is None else p * w, v).reshape(B, -1, 32 * H)
    dq, dk, dv = torch.autograd.grad(out, leaves, t["dout"].double())
    for name, want in (("out", out.detach()), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert float((r64[name] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name
    assert float((r64["lse"] - torch.logsumexp(s.detach(), -1) / math.log(2.0)).abs().max()) <= 1e-12 * float(r64["lse"].abs().max())


_FIGS = {}


def _figs(case):
    """Per output (rho, worst share of the bar) of the emulation, and its lse error: computed once per case."""
    if case["id"] not in _FIGS:
        t, r64, A = _ref(case)
        emu = MC.emulate(t, case, _weights(case))
        f = {n: (MC.rho(n, emu[n], r64[n], A[n]), float(((emu[n] - r64[n]).abs() / MC.bar(n, r64[n], A[n])).max())) for n in MC.OUTPUTS}
        f["lse"] = float((emu["lse"] - r64["lse"]).abs().max())
        _FIGS[case["id"]] = f
    return _FIGS[case["id"]]


@pytest.mark.parametrize("case", MC.CASES, ids=lambda c: c["id"])
def test_emulation_stays_inside_the_bar(case):
    _, r64, A = _ref(case)
    figs = _figs(case)
    print(case["id"], "rho, worst share of the bar:", {n: (round(figs[n][0], 3), round(figs[n][1], 3)) for n in MC.OUTPUTS})
    for n in MC.OUTPUTS:
        assert bool((A[n] >= 0).all()) and bool(r64[n].isfinite().all())
        assert figs[n][0] <= MC.RHO_EMU[n], (case["id"], n, figs)
        assert figs[n][1] <= 1.0, (case["id"], n, figs)
    assert figs["lse"] <= 1e-12 * max(1.0, float(r64["lse"].abs().max()))


def test_rho_emu_is_the_measured_maximum():
    """RHO_EMU is the measurement rounded up, not a loose cap: at most 10 % above the largest rho the table gives."""
    worst = {n: max(_figs(c)[n][0] for c in MC.CASES) for n in MC.OUTPUTS}
    print("largest rho per output:", {n: round(v, 3) for n, v in worst.items()}, "kappa:", MC.KAPPA)
    for n in MC.OUTPUTS:
        assert worst[n] <= MC.RHO_EMU[n] <= 1.1 * worst[n], (n, worst[n], MC.RHO_EMU[n])
        assert MC.KAPPA[n] == 2.0 * MC.RHO_EMU[n]


DEFECTS = [(d, cid) for d, cids in MC.DEFECT_CASES.items() for cid in cids]


@pytest.mark.parametrize("defect,cid", DEFECTS, ids=[f"{d}-{c}" for d, c in DEFECTS])
def test_bars_see_the_defect(defect, cid):
    case = MC.BY_ID[cid]
    t, r64, A = _ref(case)
    bad = MC.defective(defect, t, case)
    seen = {}
    for n in MC.OUTPUTS:
        err = (bad[n] - r64[n]).abs()
        assert bool(err.isfinite().all())
        seen[n] = float((err / MC.bar(n, r64[n], A[n])).max())
    # lse: the fp32 bar, with e_ref from the same fp32 composition run on the CPU
    le = (bad["lse"] - r64["lse"]).abs()
    seen["lse"] = float(le[le.isfinite()].max()) / MC.lse_bar(r64["lse"], MC.lse_fp32(t, case))[1]
    print(defect, cid, "largest error in units of the bar:", {n: round(v, 2) for n, v in seen.items()})
    for n in MC.DEFECT_REACH[defect]:
        assert seen[n] > 1.0, (defect, cid, n, seen)
    for n in set(MC.OUTPUTS) - set(MC.DEFECT_REACH[defect]):
        assert seen[n] == 0.0, (defect, cid, n, seen)                          # and the defect is the only difference
