"""Without a GPU: the extension ABI (include/uenc_ext.h, the entry points of csrc/ext/depth_eval.hip and their binding), the float64
restatement of tests/depth_eval_cases.py against the reference's own recorded result and against the host evaluator, the cap on
borderline threshold pixels that the GPU evaluator tests rely on, and the `accumulate` keyword of the depth evaluators."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import depth_eval_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_HEADER = os.path.join(ROOT, "include", "uenc_ext.h")
PTR = 4096          # a non-null, 16-byte aligned "address": every call below is refused before anything could read it


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cc,lang,std", [("gcc", "c", "-std=c99"), ("gcc", "c", "-std=c11"), ("g++", "c++", "-std=c++11")])
def test_ext_header_is_valid_c_and_cxx(cc, lang, std):
    r = subprocess.run([cc, "-fsyntax-only", "-x", lang, std, "-Wall", "-Wextra", "-Werror", EXT_HEADER], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ext_declarations_are_exported_and_bound_as_parsed():
    from uenc import capi
    with open(EXT_HEADER) as f:
        functions, constants = capi.parse_header(f.read())
    assert sorted(functions) == ["uenc_depth_eval_pred", "uenc_depth_eval_score", "uenc_depth_eval_ws_bytes", "uenc_na2d_tiles_per_group"]
    assert functions == capi.EXT_FUNCTIONS and constants == capi.EXT_CONSTANTS
    for name, (restype, argtypes) in functions.items():
        fn = getattr(capi.lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    c = ctypes
    assert functions["uenc_depth_eval_ws_bytes"] == (c.c_long, [c.c_int, c.c_int])
    assert functions["uenc_depth_eval_score"][1][9:11] == [c.c_double, c.c_double]
    assert functions["uenc_na2d_tiles_per_group"] == (c.c_int, [c.c_int] * 6)         # csrc/ext/na2d_plan.hip (tests/test_na2d_cases_cpu.py)
    assert constants["UENC_DEPTH_EVAL_ROW"] == 13 and constants["UENC_EXT_F64"] not in (capi.F32, capi.BF16)


def test_core_abi_is_unchanged():
    from uenc import capi
    assert len(capi.exported_symbols()) == 130 and not set(capi.EXT_FUNCTIONS) & set(capi.FUNCTIONS)
    assert not set(capi.EXT_CONSTANTS) & set(capi.CONSTANTS)
    src = open(os.path.join(ROOT, "uni-encoder-code_amd", "csrc", "ext", "depth_eval.hip")).read()
    assert '#include "../common.h"' in src and "uenc_ext.h" in src


def test_missing_ext_header_names_its_path(tmp_path):
    """A copy of the binding beside include/uenc.h but without uenc_ext.h: ImportError naming the extension header's path."""
    import importlib.util
    import shutil
    pkg = tmp_path / "a" / "b"
    pkg.mkdir(parents=True)
    (tmp_path / "include").mkdir()
    shutil.copy(os.path.join(ROOT, "include", "uenc.h"), tmp_path / "include" / "uenc.h")
    shutil.copy(os.path.join(ROOT, "uni-encoder-code_amd", "uenc", "capi.py"), pkg / "capi_copy.py")
    shutil.copy(os.path.join(ROOT, "uni-encoder-code_amd", "uenc", "libuenc_hip.so"), pkg / "libuenc_hip.so")
    spec = importlib.util.spec_from_file_location("capi_copy", pkg / "capi_copy.py")
    with pytest.raises(ImportError) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert str(tmp_path / "include" / "uenc_ext.h") in str(e.value)


def test_invalid_arguments_are_refused_without_a_gpu():
    from uenc import capi
    lib, F64 = capi.lib, capi.EXT_CONSTANTS["UENC_EXT_F64"]
    assert lib.uenc_depth_eval_ws_bytes(375, 1242) > 0
    for H, W in ((0, 5), (5, 0), (-1, 5), (65536, 65536)):
        assert lib.uenc_depth_eval_ws_bytes(H, W) < 0
    #       disp pred resized h  w  H  W  stream
    good = [PTR, PTR, None, 4, 5, 8, 9, None]
    bad = [(0, None), (1, None), (0, PTR + 2), (1, PTR + 2), (2, PTR + 2), (3, 0), (4, -1), (5, 0), (6, 0), (5, 65536)]
    for i, v in bad:
        args = list(good)
        args[i] = v
        if (i, v) == (5, 65536):
            args[6] = 65536
        assert lib.uenc_depth_eval_pred(*args) == -1, (i, v)
    ws = lib.uenc_depth_eval_ws_bytes(40, 50)
    #       gt   dtype pred H   W   r0 r1  c0 c1  min   max   ws   bytes rows row cap stream
    good = [PTR, 0, PTR, 40, 50, 2, 30, 3, 40, 1e-3, 80.0, PTR, ws, PTR, 0, 4, None]
    bad = [(0, None), (2, None), (11, None), (13, None), (0, PTR + 2), (2, PTR + 2), (11, PTR + 4), (13, PTR + 4),
           (1, 1), (1, 3), (1, -1),                                      # bf16 and unknown dtype flags
           (3, 0), (4, -2),                                              # non-positive sizes
           (5, -1), (6, 41), (5, 30), (5, 31), (7, -1), (8, 51), (7, 40), (7, 45),      # a window outside the map, or empty
           (9, 80.0), (9, float("nan")), (12, ws - 1), (14, -1), (14, 4), (15, 0)]
    for i, v in bad:
        args = list(good)
        args[i] = v
        assert lib.uenc_depth_eval_score(*args) == -1, (i, v)
    args = list(good)
    args[1], args[0] = F64, PTR + 4                                       # fp64 ground truth needs 8-byte alignment
    assert lib.uenc_depth_eval_score(*args) == -1


def test_wrappers_exist():
    from uenc import kernels as K
    for name in ("depth_eval_pred", "depth_eval_score", "depth_eval_ws"):
        assert callable(getattr(K, name))
    assert K.DEPTH_EVAL_ROW == 13 and K.DEPTH_EVAL_LAUNCHES == {torch.float32: 6, torch.float64: 10}


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------
def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "data_eval.npz"))["kitti_depth_error"]


def test_restatement_reproduces_the_references_kitti_result():
    """depth_pairs() predictions are float64 and not fp32-representable, so the restatement's arithmetic runs here on the float64 values
    (same valid set, numpy medians, clip, compute_errors: rtol 1e-12 against the reference's recorded means).  The shift that rounding
    the predictions to fp32 causes is recorded too: the GPU test feeds the rounded ones and relies on it being far inside its bound."""
    from oracle.data_eval_inputs import depth_pairs
    pairs = depth_pairs()
    assert any(not np.array_equal(p, p.astype(np.float32)) for _, p in pairs)
    rows64, rows32 = [], []
    for gt, pred in pairs:
        win = C.kitti_window(*gt.shape)
        rows64.append(C.score_f64(gt, pred, win)["row"])
        n = C.score_f64(gt, pred, win)["n"]
        rows32.append(C.score_f64(gt, pred.astype(np.float32), win)["row"])
        assert C.score_f64(gt, pred.astype(np.float32), win)["n"] == n
    np.testing.assert_allclose(np.mean(rows64, axis=0), _golden(), rtol=1e-12)
    shift = np.abs(np.mean(rows32, axis=0) - _golden()) / np.abs(_golden())
    print("relative shift of the seven means from rounding the predictions to fp32:", shift)
    assert np.all(shift[:4] < 1e-5)                                       # a tenth of the GPU test's rtol = 1e-4


@pytest.mark.parametrize("small,big", C.PRED_SHAPES)
def test_restatement_resize_agrees_with_the_host_evaluator(small, big):
    """4 ulp of fp32 at the largest tap.  The host path computes the source coordinate in fp32: at coordinate c it is off by up to
    ulp(c) = c * 2^-23, which moves the result by that times the difference of the two taps.  The bound therefore holds on maps whose
    neighbouring taps differ by a small part of the largest tap, as a disparity map's do: here a smooth field with steps below 2.5 % of
    its maximum (on white noise of the same range the host's own coordinate error alone reaches 13 ulp at 33 x 50 -> 16 x 21)."""
    from uenc.evaluation import _resize_bilinear
    g = np.random.default_rng(small[0] * 100 + big[1])
    yy, xx = np.meshgrid(np.arange(small[0]), np.arange(small[1]), indexing="ij")
    disp = (5.0 + 3.0 * np.sin(0.05 * xx + 0.03 * yy + 1.0) + g.uniform(-0.01, 0.01, small)).astype(np.float32)
    assert max(np.abs(np.diff(disp, axis=0)).max(initial=0), np.abs(np.diff(disp, axis=1)).max(initial=0)) < 0.025 * disp.max()
    want = _resize_bilinear(disp, big[1], big[0])
    got = C.resize_f64(disp, *big)
    assert got.shape == want.shape == big
    assert np.max(np.abs(got - want.astype(np.float64))) <= 4 * float(C.ulp32(disp.max()))


def test_restatement_medians_are_numpys():
    for name, (gt, pred, win) in C.score_cases().items():
        s = C.score_f64(gt, pred, win)
        r0, r1, c0, c1 = win
        inside = np.zeros(gt.shape, dtype=bool)
        inside[r0:r1, c0:c1] = True
        valid = inside & (gt > gt.dtype.type(C.MIN_DEPTH)) & (gt < gt.dtype.type(C.MAX_DEPTH))
        assert s["n"] == int(valid.sum()), name
        if s["n"]:
            assert s["med_gt"] == np.median(gt[valid].astype(np.float64)) and s["med_pred"] == np.median(pred[valid]), name
    sizes = {n: C.score_f64(*c)["n"] for n, c in C.score_cases().items()}
    assert [sizes[k] for k in ("n0", "n1", "n2", "n3", "even_middle_differs", "duplicate_straddles")] == [0, 1, 2, 3, 4, 6]
    assert sizes["bounds_f32"] == sizes["bounds_f64"] == 600 - 20 and sizes["big_f32"] > 2048 * 20


# ---- the borderline cap of the evaluator-level cases ------------------------------------------------------------------------------------------
def _assert_cap(rows, what):
    for i, (row, g, p) in enumerate(rows):
        count = C.borderline_count(g, p)
        print(f"{what} image {i}: {len(g)} valid pixels, {count} borderline, abs_rel {row[0]:.4f}")
        assert len(g) > 0 and count <= 1e-3 * len(g), (what, i, count, len(g))
        assert row[0] >= 0.05, (what, i, row[0])                          # the GPU tests' rtol rests on this


def test_borderline_cap_kitti(tmp_path):
    from uenc.evaluation import KITTIDepthEvaluator
    ev = KITTIDepthEvaluator("x")
    ev.process(*C.kitti_case(tmp_path))
    _assert_cap(C.host_rows(ev), "kitti")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_borderline_cap_cityscapes(tmp_path, dtype):
    from uenc.evaluation import CityscapesDepthEvaluator
    ev = CityscapesDepthEvaluator("x")
    ev.process(*C.cityscapes_case(tmp_path, dtype))
    rows = C.host_rows(ev)
    assert len(rows) == 2 and all(len(g) <= 8 * 1664 for _, g, _ in rows)
    _assert_cap(rows, "cityscapes")


def test_borderline_cap_depth_pairs():
    from oracle.data_eval_inputs import depth_pairs
    from uenc.evaluation import KITTIDepthEvaluator
    ev = KITTIDepthEvaluator("x")
    ev._pairs = list(depth_pairs())
    _assert_cap(C.host_rows(ev), "depth_pairs")


# ---- interface --------------------------------------------------------------------------------------------------------------------------------
def test_accumulate_keyword():
    from model import evaluation as facade
    from uenc.evaluation import CityscapesDepthEvaluator, KITTIDepthEvaluator
    assert facade.KITTIDepthEvaluator is KITTIDepthEvaluator and facade.CityscapesDepthEvaluator is CityscapesDepthEvaluator
    for cls in (KITTIDepthEvaluator, CityscapesDepthEvaluator):
        with pytest.raises(ValueError, match="accumulate"):
            cls("x", accumulate="bogus")
        assert cls("x")._accumulate == "host" and facade.__dict__[cls.__name__]("x", accumulate="device")._accumulate == "device"


def test_device_mode_refuses_host_tensors(tmp_path):
    from uenc.evaluation import CityscapesDepthEvaluator, KITTIDepthEvaluator
    inputs, outputs = C.kitti_case(tmp_path)
    with pytest.raises(ValueError, match=r'accumulate="device" counts on the GPU where the model left out\["disp_results"\]'):
        KITTIDepthEvaluator("x", accumulate="device").process(inputs[:1], outputs[:1])
    with pytest.raises(ValueError, match="it must be a GPU tensor"):
        CityscapesDepthEvaluator("x", accumulate="device").process([{"file_name": "/leftImg8bit/test/a/b.png"}], [{"disp_results": torch.zeros(1, 1, 4, 4)}])
