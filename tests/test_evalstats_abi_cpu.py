"""Argument checks of the three entry points of csrc/evalstats.hip: a null or misaligned pointer, an empty batch or a class count outside
[1, UENC_EVAL_MAX_CLASSES] is refused (-1) before any HIP call, so this runs without a GPU.  Pointers here are never dereferenced: every
call below must be refused."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from uenc import capi
    return capi.lib


PTR = 4096          # a non-null, 16-byte aligned "address" (nothing is launched, nothing reads it)
MAXC = 1024


def _refused(fn, good, pointers, bad_values):
    """`good` would be launched; each pointer null or off its natural alignment, and each (index, value) of bad_values, must give -1."""
    for i in pointers:
        for p in (None, PTR + 2):
            args = list(good)
            args[i] = p
            assert fn(*args) == -1, (i, p)
    for i, v in bad_values:
        args = list(good)
        args[i] = v
        assert fn(*args) == -1, (i, v)


def test_confusion_refuses(lib):
    #       pred gt   sizes conf B  C   H  W  N   ignore max_blocks stream
    good = [PTR, PTR, PTR, PTR, 1, 19, 8, 8, 19, 255, 0, None]
    _refused(lib.uenc_eval_confusion, good, (0, 1, 2, 3),
             [(4, 0), (4, -1), (4, 65536), (5, -1), (5, MAXC + 1), (6, 0), (6, -3), (7, 0), (8, 0), (8, -1), (8, MAXC + 1), (10, -1)])
    args = list(good)
    args[3] = PTR + 4                                                    # the int64 matrix needs 8-byte alignment
    assert lib.uenc_eval_confusion(*args) == -1
    args = list(good)
    args[6], args[7] = 65536, 65536                                      # H * W does not fit the 32-bit pixel index
    assert lib.uenc_eval_confusion(*args) == -1


def test_pq_intersect_refuses(lib):
    #       pred gt   sizes gt_ids n_gt pred_ids n_pred inter B  H  W  max_blocks stream
    good = [PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, 1, 8, 8, 0, None]
    _refused(lib.uenc_eval_pq_intersect, good, range(8), [(8, 0), (8, -2), (8, 65536), (9, 0), (9, -1), (10, 0), (11, -1)])
    args = list(good)
    args[9], args[10] = 46341, 46341
    assert lib.uenc_eval_pq_intersect(*args) == -1


def test_pq_match_refuses(lib):
    #       inter n_gt n_pred gt_cat gt_crowd pred_cat rec fp   fn   unknown B  K  stream
    good = [PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, 1, 19, None]
    _refused(lib.uenc_eval_pq_match, good, range(10), [(10, 0), (10, -1), (10, 65536), (11, 0), (11, -1), (11, MAXC + 1)])


def test_wrappers_and_constants_exist():
    from uenc import kernels as K
    for name in ("eval_confusion", "eval_pq_intersect", "eval_pq_match", "eval_pq_unpack"):
        assert callable(getattr(K, name))
    assert K.EVAL_MAX_CLASSES == MAXC and K.EVAL_PQ_DIM == K.TARGETS_MAX_SEGMENTS + 2 == 258
