"""The case table of the few-row GEMM tests is what it claims (no GPU): routes of the parent, k-range counts, tails and coverage."""
import json
import os

import gemm_fewrow_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_fewrow_parent.json")


def test_shapes_are_the_issue_table():
    assert [(c.M, c.N, c.K) for c in C.CASES] == [(1, 4, 64), (17, 36, 72), (65, 132, 136), (150, 20, 256), (1000, 136, 72), (300, 256, 256),
                                                  (298, 256, 2048), (300, 512, 256), (300, 2048, 256), (4096, 256, 256)]


def test_routes_ranges_and_tails():
    for c in C.CASES:
        assert c.K % 8 == 0 and c.K >= 64 and c.N % 4 == 0 and c.M >= 1
        assert C.parent_route(c.M, c.N, c.K) == c.route, c
        rs = C.k_ranges(c.K)
        per32 = rs[1][0]
        assert sum(e <= b for b, e in rs) == c.empty, c
        assert sum(b < e < b + per32 for b, e in rs) == c.partial, c
        # the ranges tile [0, K) in order
        covered = [k for b, e in rs for k in range(b, e)]
        assert covered == list(range(c.K)), c
        assert ("m" in c.tails) == (c.M % 16 != 0) and ("n8" in c.tails) == (c.N % 8 != 0) and ("k32" in c.tails) == (c.K % 32 != 0), c


def test_coverage():
    allv = C.all_variants()
    assert len(allv) == 4 * len(C.CASES)
    for ci in range(len(C.CASES)):
        assert sorted((v.a_f32, v.out_f32) for v in C.variants(ci)) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    vs = [v for _, _, v in allv]
    assert {v.epi for v in vs} == {0, 1, 2, 3, 4, 5}
    for v in vs:        # what the small-shape kernels take
        assert v.epi in ((0, 2, 3) if v.out_f32 else (0, 1, 2, 4, 5))
        assert v.aux_out <= (v.epi == C.EPI_GELU)
    assert any(v.aux_out for v in vs) and any(v.epi == C.EPI_GELU and not v.aux_out for v in vs)
    assert any(v.bias for v in vs) and any(not v.bias for v in vs)
    assert any(v.alpha == 0.5 for v in vs)
    assert any(v.a_slice and v.a_f32 for v in vs) and any(v.a_slice and not v.a_f32 for v in vs)
    assert any(v.out_slice and v.out_f32 for v in vs) and any(v.out_slice and not v.out_f32 for v in vs)
    scaled = [(C.CASES[ci], v) for ci, _, v in allv if v.scale]
    assert scaled and all(c.M == 300 for c, _ in scaled)
    # both summation orders see the residual epilogue, the strided output and the fp32 A
    for route in ("skinny", "tile128"):
        rv = [v for ci, _, v in allv if C.CASES[ci].route == route]
        assert any(v.epi == C.EPI_RESIDUAL for v in rv) and any(v.out_slice for v in rv) and any(v.a_f32 for v in rv)
    assert len({C.variant_id(ci, vi) for ci, vi, _ in allv}) == len(allv)


def test_golden_lists_every_call_and_its_inputs():
    with open(GOLDEN) as f:
        gold = json.load(f)["cases"]
    assert sorted(gold) == sorted(C.variant_id(ci, vi) for ci, vi, _ in C.all_variants())
    for ci, vi, _ in C.all_variants():
        if C.CASES[ci].M * C.CASES[ci].N <= 40000:       # (the small ones: the generator check proper runs with the GPU test)
            assert C.inputs_hash(C.make_inputs(ci, vi)) == gold[C.variant_id(ci, vi)]["inputs"], C.variant_id(ci, vi)
