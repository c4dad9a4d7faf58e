"""The few-row NT GEMM kernel (csrc/gemm.hip: gemm_nt_fewrow_kernel) over the case table of gemm_fewrow_cases.py: every element written
and nothing else, results bit-identical to the parent commit's kernels (tests/golden/gemm_fewrow_parent.json, recorded there by
tools/gemm_fewrow_identity.py), close to the float64 product of the bf16-rounded operands, and one kind-0 launch per call.

Tolerances are those of tests/test_kernels_gpu.py for these operand scales (weights scaled by K ** -0.5): 2e-2 / 1e-2 for bf16
outputs (one 2^-9 relative rounding of O(1) values), 2e-3 / 2e-3 for fp32 outputs."""
import ctypes
import json
import os

import pytest
import torch

import gemm_fewrow_cases as C

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_fewrow_parent.json")
IDS = [C.variant_id(ci, vi) for ci, vi, _ in C.all_variants()]


@pytest.fixture(scope="module")
def K():
    from uenc import kernels
    return kernels


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def runs(K):
    """Every call of the table, run once with the launch timers on: id -> (inputs, padded output, window, aux_out, kind-0 launches)."""
    from uenc.capi import lib
    out = {}
    for ci, vi, _ in C.all_variants():
        inp = C.make_inputs(ci, vi)
        lib.uenc_prof_enable(1)
        try:
            buf, win, aux_out = C.run_variant(K, ci, vi, inp)
            torch.cuda.synchronize()
            n = ctypes.c_long()
            lib.uenc_prof_collect(0, None, None, ctypes.byref(n))
            others = []
            for kind in (1, 4, 5):
                k = ctypes.c_long()
                lib.uenc_prof_collect(kind, None, None, ctypes.byref(k))
                others.append(k.value)
        finally:
            lib.uenc_prof_enable(0)
        out[C.variant_id(ci, vi)] = (ci, vi, inp, buf, win, aux_out, n.value, others)
    return out


@pytest.mark.parametrize("vid", IDS)
def test_sentinels(runs, vid):
    ci, vi, inp, buf, (lo, hi), aux_out, _, _ = runs[vid]
    b = buf.float().cpu()
    assert not torch.isnan(b[:, lo:hi]).any(), "an output element was not written"
    assert torch.isnan(b[:, :lo]).all() and torch.isnan(b[:, hi:]).all(), "written outside the M x N window"
    if aux_out is not None:
        assert not torch.isnan(aux_out.float()).any()


@pytest.mark.parametrize("vid", IDS)
def test_identical_to_parent(runs, gold, vid):
    ci, vi, inp, buf, win, aux_out, _, _ = runs[vid]
    assert C.inputs_hash(inp) == gold[vid]["inputs"], "the seeded inputs differ from the recorded ones: generator difference, not a kernel one"
    assert C.outputs_hash(buf, win, aux_out) == gold[vid]["outputs"]


@pytest.mark.parametrize("vid", IDS)
def test_against_float64(runs, vid):
    ci, vi, inp, buf, (lo, hi), aux_out, _, _ = runs[vid]
    v = C.variants(ci)[vi]
    pre, want = C.reference(ci, vi, inp)
    atol, rtol = (2e-3, 2e-3) if v.out_f32 else (2e-2, 1e-2)
    torch.testing.assert_close(buf[:, lo:hi].double().cpu(), want, atol=atol, rtol=rtol)
    if aux_out is not None:
        torch.testing.assert_close(aux_out.double().cpu(), pre, atol=2e-2, rtol=1e-2)


@pytest.mark.parametrize("vid", IDS)
def test_one_kind0_launch(runs, vid):
    *_, n, others = runs[vid]
    assert n == 1 and others == [0, 0, 0]
