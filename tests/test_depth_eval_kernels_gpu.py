"""The two entry points of csrc/ext/depth_eval.hip against the float64 restatement of depth_eval_cases.py, at the smallest shapes that reach
each branch: every resize direction, and for the score every size of valid set at which the radix select or the reduction takes
another path (none, one, two, three, an even count, one bin at every pass, the last digit only, fp64 below fp32 precision, duplicates
over the median rank, several workgroups, windows on every border, the strict depth bounds)."""
import numpy as np
import pytest
import torch

import depth_eval_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from uenc import kernels
    return kernels


@pytest.fixture(scope="module")
def cases():
    return C.score_cases()


# ---- pred --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small,big", C.PRED_SHAPES)
def test_pred_is_the_restatement_rounded_once(K, small, big):
    g = np.random.default_rng(small[0] * 1000 + big[1])
    disp = g.uniform(0.01, 10.0, small).astype(np.float32)
    pred, resized = K.depth_eval_pred(torch.from_numpy(disp).cuda(), big, want_resized=True)
    resized, pred = resized.cpu().numpy(), pred.cpu().numpy()
    want, _ = C.pred_f32(disp, *big)
    assert resized.shape == pred.shape == big
    # the kernel may contract a lerp into an fma: its float64 value differs from numpy's in the last bits, so the one rounding to fp32
    # may fall on the other side.  At most 1 ulp of fp32; nothing else is permitted.
    err = np.abs(resized.astype(np.float64) - want.astype(np.float64))
    assert np.all(err <= C.ulp32(want)), float((err / C.ulp32(want)).max())
    assert np.mean(resized == want) > 0.99
    assert np.array_equal(pred.view(np.uint32), (np.float32(1.0) / resized).view(np.uint32))      # IEEE division of the device's own value
    assert np.array_equal(K.depth_eval_pred(torch.from_numpy(disp).cuda(), big).cpu().numpy(), pred)


# ---- score -------------------------------------------------------------------------------------------------------------------------------
def _score(K, gt, pred, win, rows=None, row=0):
    if rows is None:
        rows = torch.zeros((1, K.DEPTH_EVAL_ROW), dtype=torch.float64, device="cuda")
    K.depth_eval_score(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), win, C.MIN_DEPTH, C.MAX_DEPTH, rows, row)
    return rows


def _bits(a):
    return np.asarray(a).view(np.uint64 if np.asarray(a).dtype == np.float64 else np.uint32)


def _check(name, got, want):
    """got: one device row; want: score_f64.  Medians bit-equal, n and the three counts equal as integers, the continuous metrics within
    rtol = 1e-9.  Derivation: each of the four sums has at most 2^20 positive terms (the largest window the evaluators score is
    512 x 1664 < 2^20); summed in fp64 in any order the relative error is below 2^20 * 2^-53 = 2^-33 = 1.2e-10; every term is a few
    fp64 operations and, for rmse_log, two logs accurate to a few ulp whose difference is squared: a few 2^-53 relative to terms
    that do not cancel in a sum of squares.  1e-9 covers 2^-33 with an eightfold margin; the square roots halve the error."""
    n = want["n"]
    assert got[7] == n, name
    if n == 0:
        assert np.all(np.isnan(got[:7])) and np.isnan(got[8]) and np.isnan(got[9]) and np.all(got[10:13] == 0), name
        return
    assert _bits(np.float64(got[8])) == _bits(np.float64(want["med_gt"])), (name, got[8], want["med_gt"])
    assert got[9] == np.float64(want["med_pred"]) and _bits(np.float32(got[9])) == _bits(want["med_pred"]), (name, got[9], want["med_pred"])
    assert [int(v) for v in got[10:13]] == list(want["counts"]) and np.all(got[10:13] == np.round(got[10:13])), name
    np.testing.assert_array_equal(got[4:7], want["counts"] / n, err_msg=name)
    np.testing.assert_allclose(got[:4], want["row"][:4], rtol=1e-9, atol=0, err_msg=name)


def test_score_cases(K, cases):
    """All cases in one test: each is six to ten tiny launches; the restatement is computed once per case."""
    rows = torch.full((len(cases), K.DEPTH_EVAL_ROW), -7.0, dtype=torch.float64, device="cuda")
    for i, (gt, pred, win) in enumerate(cases.values()):
        _score(K, gt, pred, win, rows, i)
    got = rows.cpu().numpy()
    for i, (name, (gt, pred, win)) in enumerate(cases.items()):
        _check(name, got[i], C.score_f64(gt, pred, win))
    assert got[list(cases).index("n0"), 7] == 0 and got[list(cases).index("big_f32"), 7] > 2048 * 20


def test_score_after_the_devices_own_pred(K):
    """pred -> score as the evaluator chains them: the restatement is fed the device's own fp32 prediction."""
    g = np.random.default_rng(5)
    gt = g.uniform(0.0, 100.0, (40, 120))
    gt[g.uniform(size=gt.shape) < 0.5] = 0.0
    disp = (1.0 / (np.where(C._low_res(gt, 12, 40) > 0, C._low_res(gt, 12, 40), 10.0) * 0.5)).astype(np.float32)
    pred = K.depth_eval_pred(torch.from_numpy(disp).cuda(), (40, 120))
    win = C.kitti_window(40, 120)
    for dt in (np.float32, np.float64):
        rows = torch.zeros((1, K.DEPTH_EVAL_ROW), dtype=torch.float64, device="cuda")
        K.depth_eval_score(torch.from_numpy(gt.astype(dt)).cuda(), pred, win, C.MIN_DEPTH, C.MAX_DEPTH, rows, 0)
        _check(str(dt), rows.cpu().numpy()[0], C.score_f64(gt.astype(dt), pred.cpu().numpy(), win))


def test_score_is_bit_reproducible(K, cases):
    for name in ("big_f32", "big_f64", "window_whole"):
        a = _score(K, *cases[name]).cpu().numpy()
        b = _score(K, *cases[name]).cpu().numpy()
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), name


def test_score_writes_only_its_row(K, cases):
    rows = torch.full((7, K.DEPTH_EVAL_ROW), -3.0, dtype=torch.float64, device="cuda")
    ws = K.depth_eval_ws(40, 50, "cuda")                                  # one workspace, reused by consecutive calls on one stream
    names = {0: "window_top", 1: "window_one_row", 5: "window_whole"}
    for r, name in names.items():
        gt, pred, win = cases[name]
        K.depth_eval_score(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), win, C.MIN_DEPTH, C.MAX_DEPTH, rows, r, ws)
    got = rows.cpu().numpy()
    for r in range(7):
        if r in names:
            _check(names[r], got[r], C.score_f64(*cases[names[r]]))
        else:
            assert np.all(got[r] == -3.0), r


def test_wrapper_refuses_what_does_not_fit(K):
    from uenc.capi import UencError
    rows = torch.zeros((2, K.DEPTH_EVAL_ROW), dtype=torch.float64, device="cuda")
    gt, pred = torch.ones((8, 9), device="cuda"), torch.ones((8, 9), device="cuda")
    for bad in (dict(window=(0, 9, 0, 9)), dict(window=(3, 3, 0, 9)), dict(row=2), dict(gt=gt.half()), dict(pred=pred[:, :8].contiguous())):
        kw = dict(gt=gt, pred=pred, window=(0, 8, 0, 9), min_depth=C.MIN_DEPTH, max_depth=C.MAX_DEPTH, rows=rows, row=0)
        kw.update(bad)
        with pytest.raises(UencError):
            K.depth_eval_score(**kw)
