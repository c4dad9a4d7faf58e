"""Argument checks of the entry points of csrc/augment.hip: null or misaligned pointers, zero sizes, a window outside the resized image
and a plan whose LDS tile would not fit are refused (-1) before any HIP call, so this runs without a GPU.  Pointers here are never
dereferenced: every call below must be refused, no launch is made."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from uenc import capi
    return capi.lib


PTR = 4096          # a non-null, 16-byte aligned "address"

#             src  stride F  in_h in_w rs_h rs_w x0 y0 cw  ch  col  kx row  ky ctab flags hue flip out_h out_w pad dst  stream
IMAGE_GOOD = [PTR, 4608, 1, 24, 48, 12, 24, 2, 1, 20, 10, PTR, 5, PTR, 5, PTR, 7, 6, 0, 10, 20, 128, PTR, None]
#              pan  label bytes in_h in_w rs_h rs_w x0 y0 cw  ch  pcol prow lcol lrow flip out_h out_w ignore pan_out lab_out stream
LABELS_GOOD = [PTR, PTR, 1, 24, 48, 12, 24, 2, 1, 20, 10, PTR, PTR, PTR, PTR, 0, 10, 20, 255, PTR, PTR, None]


def _refused(fn, good, changes):
    for i, v in changes:
        args = list(good)
        args[i] = v
        assert fn(*args) == -1, (i, v)


def test_image_refuses(lib):
    fn = lib.uenc_augment_image
    _refused(fn, IMAGE_GOOD, [(0, None), (11, None), (13, None), (22, None), (11, PTR + 2), (13, PTR + 1), (15, PTR + 2)])     # pointers
    _refused(fn, IMAGE_GOOD, [(2, 0), (2, -1), (2, 65536), (3, 0), (4, 0), (4, -5), (5, 0), (6, 0), (9, 0), (10, 0), (9, -3), (19, 0), (20, 0),
                              (19, -1), (1, 100)])                                                                             # sizes
    _refused(fn, IMAGE_GOOD, [(7, -1), (8, -1), (7, 5), (8, 3), (9, 23), (10, 12), (7, 1 << 30)])                              # the window
    _refused(fn, IMAGE_GOOD, [(12, 0), (14, 0), (12, 8), (14, 9), (16, 16), (16, -1), (17, 180), (17, -180), (18, 2), (21, 256), (21, -1)])
    args = list(IMAGE_GOOD)
    args[15], args[16] = None, 3                                             # colour stages without a colour table
    assert fn(*args) == -1


def test_image_refuses_a_tile_that_does_not_fit(lib):
    fn = lib.uenc_augment_image
    # x0.25 along the width: 63 * 4 + 9 + 1 source pixels per tile > 165 (and 9 taps > 7)
    wide = list(IMAGE_GOOD)
    wide[3], wide[4], wide[5], wide[6], wide[1] = 24, 640, 24, 160, 24 * 640 * 3
    wide[7], wide[8], wide[9], wide[10], wide[12] = 0, 0, 160, 24, 7
    assert fn(*wide) == -1
    # x0.25 along the height: 15 * 4 + 7 + 1 source rows per tile > 40
    tall = list(IMAGE_GOOD)
    tall[3], tall[4], tall[5], tall[6], tall[1] = 256, 48, 64, 48, 256 * 48 * 3
    tall[7], tall[8], tall[9], tall[10], tall[12], tall[14] = 0, 0, 48, 64, 3, 7
    assert fn(*tall) == -1
    assert lib.uenc_augment_tile_fits(1024, 2048, 512, 1024, 5, 5) == 1      # the smallest configured scale (SEG_MIN_SIZE_TRAIN 512)
    assert lib.uenc_augment_tile_fits(1024, 2048, 2048, 4096, 3, 3) == 1      # the largest
    assert lib.uenc_augment_tile_fits(1024, 2048, 1024, 2048, 3, 3) == 1
    assert lib.uenc_augment_tile_fits(1024, 2048, 256, 512, 7, 7) == 0
    assert lib.uenc_augment_tile_fits(24, 48, 12, 24, 8, 5) == 0 and lib.uenc_augment_tile_fits(24, 48, 12, 24, 5, 0) == 0
    assert lib.uenc_augment_tile_fits(0, 48, 12, 24, 5, 5) == 0 and lib.uenc_augment_tile_fits(24, 48, 12, 0, 5, 5) == 0


def test_labels_refuses(lib):
    fn = lib.uenc_augment_labels
    _refused(fn, LABELS_GOOD, [(0, None), (11, None), (12, None), (19, None), (13, None), (14, None), (11, PTR + 2), (12, PTR + 2), (13, PTR + 1),
                               (14, PTR + 3), (19, PTR + 2), (20, PTR + 2)])
    _refused(fn, LABELS_GOOD, [(1, None), (20, None)])                       # a label map without its output, and the reverse
    _refused(fn, LABELS_GOOD, [(2, 0), (2, 2), (2, 8), (3, 0), (4, 0), (5, 0), (6, 0), (9, 0), (10, 0), (16, 0), (17, 0), (17, -2), (15, 2), (15, -1)])
    _refused(fn, LABELS_GOOD, [(7, -1), (8, -1), (7, 5), (8, 3), (9, 23), (10, 12)])
    args = list(LABELS_GOOD)
    args[1], args[2] = PTR + 2, 4                                            # an int32 label map off its alignment
    assert fn(*args) == -1


def test_wrappers_and_constants_exist():
    from uenc import kernels as K
    for name in ("augment_image", "augment_labels", "augment_sample", "augment_tile_fits"):
        assert callable(getattr(K, name))
    assert (K.AUG_TILE_W, K.AUG_TILE_H, K.AUG_MAX_TAPS, K.AUG_COLOUR_TAB_INTS) == (64, 16, 7, 704)
    assert K.augment_tile_fits(1024, 2048, 512, 1024, 5, 5) and not K.augment_tile_fits(1024, 2048, 256, 512, 7, 7)
