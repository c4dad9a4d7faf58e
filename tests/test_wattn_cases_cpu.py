"""The cases, references and bars of tests/wattn_cases.py, checked without a GPU: the table against what each case claims to reach, the
step-by-step reference against the oracle's gather layout and against the window-domain closed forms, the emulation inside the bar with
rho <= RHO_EMU (which fixes kappa), emu32 with rho32 <= RHO32 (which fixes gamma) and the gamma cap, and the defects the bars must see."""
import pytest
import torch

import wattn_cases as WC

_REF = {}


def _ref(case):
    """(inputs, r64, closed forms, A, emulation, emu32) of one case: computed once per module and left unchanged."""
    if case["id"] not in _REF:
        t = WC.inputs(case)
        cf, A = WC.windowed(t, case)
        _REF[case["id"]] = (t, WC.reference(t, case), cf, A, WC.emulate(t, case), WC.reference(t, case, torch.float32))
    return _REF[case["id"]]


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    _REF.clear()


def test_case_table_is_well_formed():
    ids = [c["id"] for c in WC.CASES]
    assert len(set(ids)) == len(ids)
    for c in WC.CASES:
        assert 1 <= c["ws"] <= 12 and 0 <= c["shift"] < c["ws"], c["id"]
        assert WC.n_scores(c) <= WC.MAX_SCORES, c["id"]
        assert c["B"] * c["H"] * c["W"] * 96 * c["nH"] < 2 ** 31, c["id"]              # the kernels' 32-bit token offsets
    # every instantiation a window size can reach (NT = 5 has none), and every window size
    reachable = {WC.ntiles(ws) for ws in range(1, 13)}
    assert reachable == {1, 2, 3, 4, 6, 7, 8, 9}
    assert {WC.ntiles(c["ws"]) for c in WC.CASES} == reachable
    assert {c["ws"] for c in WC.CASES} == set(range(1, 13))
    assert all(set(v) <= set(WC.BY_ID) for v in WC.DEFECT_CASES.values()) and set(WC.DEFECT_CASES) == set(WC.DEFECT_REACH)


def test_case_table_reaches_what_it_names():
    C = WC.BY_ID
    pad = lambda c: bool((WC.layout(c)[0] == c["H"] * c["W"]).any())
    G = lambda c: WC.bwd_groups(c["B"], c["H"], c["W"], c["nH"], c["ws"])
    # a: N = 1, a forward grid that rounds up
    assert C["a-ws1"]["ws"] == 1 and WC.n_windows(C["a-ws1"]) == 15
    # padding on both axes / none at all / N == NP
    for i in ("b-ws2", "d-ws5", "k-ws12-s0", "k-ws12-s6"):
        assert C[i]["H"] % C[i]["ws"] and C[i]["W"] % C[i]["ws"] and pad(C[i])
    for i in ("c-ws4", "g-ws8", "n-g5", "n-g16", "o-batch", "a-ws1"):
        assert not pad(C[i])
    for i in ("c-ws4", "g-ws8", "k-ws12-s0", "n-g5"):
        assert C[i]["ws"] ** 2 == 16 * WC.ntiles(C[i]["ws"])
    assert C["b-ws2"]["B"] == 2 and C["c-ws4"]["nH"] % 2 == 1 and C["f-ws7"]["nH"] % 2 == 1
    # the instantiations no test launched before, the odd tile counts, the three targets of the group heuristic
    assert [WC.ntiles(C[i]["ws"]) for i in ("e-ws6", "h-ws9", "i-ws10", "j-ws11")] == [3, 6, 7, 8]
    assert {WC.ntiles(c["ws"]) for c in WC.CASES} >= {1, 3, 7, 9}
    # the group count is capped by the windows in the small cases: the targets themselves are reached where heads are many
    assert G(C["n-g5"]) == 256 // 48 and G(C["n-g16"]) == 512 // 32
    # padding-dominated windows: one real token among 144 slots; 6 among 49
    src = WC.layout(C["l-one-token"])[0]
    assert src.shape == (1, 144) and int((src < 1).sum()) == 1
    src = WC.layout(C["l-ws7-pad"])[0]
    assert src.shape == (1, 49) and int((src < 6).sum()) == 6 and C["l-ws7-pad"]["shift"] > 0
    # Hp == ws / Wp == ws with a shift: the first slice of that axis is empty, two regions remain on it
    c = C["m-hp-eq-ws"]
    assert WC.padded(c)[0] == c["ws"] and WC.padded(c)[1] > c["ws"] and c["shift"] > 0
    assert sorted(WC.region_map(c).unique().tolist()) == [3, 4, 5, 6, 7, 8]
    c = C["m-wp-eq-ws"]
    assert WC.padded(c)[1] == c["ws"] and WC.padded(c)[0] > c["ws"] and c["shift"] > 0
    assert sorted(WC.region_map(c).unique().tolist()) == [1, 2, 4, 5, 7, 8]
    # several windows per persistent workgroup
    assert WC.n_windows(C["n-g5"]) == 18 and WC.windows_per_group(C["n-g5"]) == [4, 4, 4, 3, 3]
    assert WC.n_windows(C["n-g16"]) == 24 and WC.windows_per_group(C["n-g16"]) == [2] * 8 + [1] * 8
    assert C["n-g5"]["ws"] == 12 and C["n-g5"]["shift"] > 0 and WC.ntiles(C["n-g16"]["ws"]) <= 8
    # o: 18 windows over three images, not a multiple of 8
    assert C["o-batch"]["B"] == 3 and WC.n_windows(C["o-batch"]) == 18
    # with and without a shift at 12 x 12
    assert {c["shift"] for c in WC.CASES if c["ws"] == 12} == {0, 6}
    # the tail-key defect needs N < NP, the boundary defect 0 < shift < ws - 1
    assert all(C[i]["ws"] ** 2 < 16 * WC.ntiles(C[i]["ws"]) for i in WC.DEFECT_CASES["f_tail_keys_admitted"])
    assert all(0 < C[i]["shift"] < C[i]["ws"] - 1 for i in WC.DEFECT_CASES["b_mask_boundary_off_by_one"])


def test_group_heuristic_restated():
    assert WC.bwd_groups(2, 96, 120, 6, 12) == 42 and WC.bwd_groups(2, 40, 50, 24, 12) == 10 and WC.bwd_groups(2, 42, 42, 16, 7) == 32
    assert WC.bwd_groups(1, 8, 8, 2048, 4) == 1 and WC.bwd_groups(1, 4, 4, 1, 4) == 1
    assert WC.ws_floats(1, 36, 72, 48, 12) == 48 * 5 * 144 * 144


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c["id"])
def test_layout_equals_the_oracle(case):
    """pad / roll / partition on an index map, and the img_mask slices, against oracle.torch_ref.window_layout's index arithmetic."""
    from oracle import torch_ref as T
    src, rid = WC.layout(case)
    osrc, orid = T.window_layout(case["H"], case["W"], case["ws"], case["shift"])
    assert torch.equal(src, osrc)
    # region numbers may be labelled differently; what the mask needs is the same partition of every window's slots
    assert torch.equal(rid[:, :, None] != rid[:, None, :], orid[:, :, None] != orid[:, None, :])
    assert torch.equal(WC.relative_position_index(case["ws"]), T.relative_position_index(case["ws"]))


@pytest.mark.parametrize("cid", ["b-ws2", "d-ws5", "m-hp-eq-ws", "k-ws12-s6", "l-one-token", "o-batch"])
def test_reference_equals_the_oracle_gather(cid):
    """r64 (roll and partition on the data) against the gather / scatter statement tests/test_kernels_gpu.py judges the kernels by, in
    float64 with its own autograd."""
    from test_kernels_gpu import _window_attn_ref
    case = WC.BY_ID[cid]
    t, r64 = _ref(case)[:2]
    leaves = [t[n].double().requires_grad_(True) for n in ("qkv", "qkv_bias", "table")]
    out = _window_attn_ref(*leaves, case["H"], case["W"], case["ws"], case["shift"], case["nH"])
    grads = torch.autograd.grad(out, leaves, t["dout"].double(), allow_unused=True)
    for name, want in (("out", out.detach()), ("dqkv", grads[0]), ("dpad", grads[1]), ("dtable", grads[2])):
        assert float((r64[name] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c["id"])
def test_closed_forms_equal_autograd(case):
    """The window-domain closed forms the emulation and the defects are built on, unrounded, against r64; lse too."""
    _, r64, cf, A, _, _ = _ref(case)
    for n in WC.OUTPUTS + ("lse",):
        assert cf[n].shape == r64[n].shape
        assert float((cf[n] - r64[n]).abs().max()) <= 1e-12 * max(1.0, float(r64[n].abs().max())), n
    for n in WC.OUTPUTS:
        assert A[n].shape == r64[n].shape and bool((A[n] >= 0).all()) and bool((A[n] >= r64[n].abs() * (1 - 1e-9)).all()), n
    if case["ws"] == 1:                                                              # one key: out is v
        C = 32 * case["nH"]
        assert torch.equal(r64["out"], _ref(case)[0]["qkv"][..., 2 * C:].double())


_FIGS = {}


def _figs(case):
    if case["id"] not in _FIGS:
        _, r64, _, A, emu, e32 = _ref(case)
        _FIGS[case["id"]] = dict(
            rho={n: WC.rho(n, emu[n], r64[n], A[n]) for n in WC.OUTPUTS}, rho32={n: WC.rho32(n, e32[n], r64[n], A[n]) for n in WC.OUTPUTS},
            share={n: float(((emu[n] - r64[n]).abs() / WC.bar(n, r64[n], A[n])).max()) for n in WC.OUTPUTS},
            share32={n: float(((e32[n].double() - r64[n]).abs() / WC.bar32(n, r64[n], A[n])).max()) for n in WC.OUTPUTS},
            lse=float((emu["lse"] - r64["lse"]).abs().max()))
    return _FIGS[case["id"]]


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c["id"])
def test_emulations_stay_inside_the_bars(case):
    r64 = _ref(case)[1]
    f = _figs(case)
    print(case["id"], {k: {n: round(v, 3) for n, v in f[k].items()} for k in ("rho", "share", "rho32", "share32")})
    for n in WC.OUTPUTS:
        assert bool(r64[n].isfinite().all())
        assert f["rho"][n] <= WC.RHO_EMU[n] and f["share"][n] <= 1.0, (case["id"], n, f)
        assert f["rho32"][n] <= WC.RHO32[n] and f["share32"][n] <= 1.0, (case["id"], n, f)
    assert f["lse"] <= 1e-12 * max(1.0, float(r64["lse"].abs().max()))            # no rounding point touches the statistics


def test_rho_is_the_measured_maximum():
    """RHO_EMU and RHO32 are the measurements rounded up, not loose caps: at most 10 % above the largest ratio the table gives; gamma
    2^-24 stays below 2^-14 -- beyond that the fp32 bar would no longer be an fp32-level bar and its margin would have to be derived
    again, not widened."""
    for key, table, factor, mult in (("rho", WC.RHO_EMU, 2.0, WC.KAPPA), ("rho32", WC.RHO32, 8.0, WC.GAMMA)):
        worst = {n: max(_figs(c)[key][n] for c in WC.CASES) for n in WC.OUTPUTS}
        print("largest", key, {n: round(v, 3) for n, v in worst.items()}, mult)
        for n in WC.OUTPUTS:
            assert worst[n] <= table[n] <= 1.1 * worst[n], (key, n, worst[n], table[n])
            assert mult[n] == factor * table[n]
    assert max(WC.GAMMA.values()) * WC.U24 < 2.0 ** -14


def test_lse_against_an_independent_fp32_composition():
    """r64's lse against log2(e) * logsumexp of scores gathered with the oracle's layout and composed in fp32: the difference is fp32
    rounding of a 32-term dot product and of the statistics -- (32 + 4) 2^-24 of the largest absolute score contraction plus 4 ulp."""
    from oracle import torch_ref as T
    for cid in ("d-ws5", "k-ws12-s6", "l-ws7-pad"):
        case = WC.BY_ID[cid]
        t, r64 = _ref(case)[:2]
        B, H, W, nH, ws, shift = (case[n] for n in ("B", "H", "W", "nH", "ws", "shift"))
        L, C, N = H * W, 32 * nH, ws * ws
        src, rid = T.window_layout(H, W, ws, shift)
        z = torch.cat([t["qkv"].float(), t["qkv_bias"].float().expand(B, 1, 3 * C)], 1)[:, src.reshape(-1)]
        q, k = (z[..., i * C:(i + 1) * C].reshape(B, -1, N, nH, 32).transpose(2, 3) for i in (0, 1))
        bias = t["table"][T.relative_position_index(ws).reshape(-1)].view(N, N, nH).permute(2, 0, 1)
        s = torch.einsum("bwhqd,bwhkd->bwhqk", q, k) * WC.SCALE + bias
        bound = WC.SCALE * float(torch.einsum("bwhqd,bwhkd->bwhqk", q.abs(), k.abs()).max()) + float(bias.abs().max())
        if shift > 0:
            s = s + ((rid[:, :, None] != rid[:, None, :]).float() * -100.0)[None, :, None]
            bound += 100.0
        lse = (torch.logsumexp(s, -1) * WC.LOG2E).transpose(2, 3).reshape(B, -1, nH)          # (B, nW N, nH)
        got = torch.zeros(B, L + 1, nH).index_copy_(1, src.reshape(-1), lse)[:, :L]
        err = float((got.double() - r64["lse"]).abs().max())
        assert err <= WC.LOG2E * 36 * WC.U24 * bound + 4 * WC.U24 * float(r64["lse"].abs().max()), (cid, err)
        assert err > 0.0


DEFECTS = [(d, cid) for d, cids in WC.DEFECT_CASES.items() for cid in cids]


@pytest.mark.parametrize("defect,cid", DEFECTS, ids=[f"{d}-{c}" for d, c in DEFECTS])
def test_bars_see_the_defect(defect, cid):
    """The defect applied to the emulation: every output it must reach leaves its bar, every output it cannot reach keeps its bits.  The
    two defects with an empty reach are the ones tests/wattn_cases.py documents as within the bar: they must stay inside it here, so
    that the documentation cannot go stale unnoticed."""
    case = WC.BY_ID[cid]
    t, r64, _, A, emu, e32 = _ref(case)
    bad = WC.emulate(t, case, defect)
    seen = {}
    for n in WC.OUTPUTS:
        err = (bad[n] - r64[n]).abs()
        assert bool(err.isfinite().all())
        seen[n] = float((err / WC.bar(n, r64[n], A[n])).max())
    seen["lse"] = float((bad["lse"] - r64["lse"]).abs().max()) / WC.lse_bar(r64["lse"], e32["lse"])[1]
    print(defect, cid, "largest error in units of the bar:", {n: round(v, 2) for n, v in seen.items()})
    for n in WC.DEFECT_REACH[defect]:
        assert seen[n] > 1.0, (defect, cid, n, seen)
    for n in WC.DEFECT_UNTOUCHED.get(defect, ()):
        assert torch.equal(bad[n], emu[n]), (defect, cid, n)
    if not WC.DEFECT_REACH[defect]:
        assert all(v <= 1.0 for v in seen.values()), (defect, cid, seen)
