"""Argument checks of the six entry points of csrc/depth_head.hip: a bad shape, dtype tag or pointer is refused (-1) before any HIP call,
so this runs without a GPU.  Pointers here are never dereferenced: every call below must be refused."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from uenc import capi
    return capi.lib


PTR = 4096          # a non-null, 16-byte aligned "address" (nothing is launched, nothing reads it)
F32, BF16 = 0, 1


def test_upsample_refuses(lib):
    for fn in (lib.uenc_upsample2x_ac_fwd, lib.uenc_upsample2x_ac_bwd):
        assert fn(None, F32, PTR, F32, 1, 4, 4, 8, None) == -1                  # null input
        assert fn(PTR, F32, None, F32, 1, 4, 4, 8, None) == -1                  # null output
        assert fn(PTR, F32, PTR, F32, 1, 4, 4, 12, None) == -1                  # C % 8 != 0
        assert fn(PTR, F32, PTR, F32, 1, 4, 4, 0, None) == -1
        assert fn(PTR, F32, PTR, F32, 0, 4, 4, 8, None) == -1
        assert fn(PTR, F32, PTR, F32, 1, 0, 4, 8, None) == -1
        assert fn(PTR, 2, PTR, F32, 1, 4, 4, 8, None) == -1                     # unknown dtype tag
        assert fn(PTR + 4, F32, PTR, F32, 1, 4, 4, 8, None) == -1               # misaligned


def test_softmax_gate_refuses(lib):
    f, b = lib.uenc_softmax_gate_fwd, lib.uenc_softmax_gate_bwd
    assert f(PTR, F32, PTR, F32, PTR, F32, PTR, PTR, F32, 4, 12, None) == -1    # C % 8 != 0
    assert f(PTR, F32, PTR, F32, PTR, F32, PTR, PTR, F32, 4, 2056, None) == -1  # wider than a wave holds
    assert f(PTR, F32, PTR, F32, PTR, F32, PTR, PTR, F32, 0, 256, None) == -1
    for i in (0, 2, 4, 6, 7):                                                  # each pointer null in turn
        args = [PTR, F32, PTR, F32, PTR, F32, PTR, PTR, F32, 4, 256, None]
        args[i] = None
        assert f(*args) == -1
    assert f(PTR, F32, PTR, 3, PTR, F32, PTR, PTR, F32, 4, 256, None) == -1
    assert b(PTR, F32, None, 0, PTR, F32, PTR, F32, PTR, PTR, F32, 4, 12, None) == -1
    assert b(PTR, F32, None, 0, PTR, F32, PTR, F32, PTR, PTR, F32, 4, 2056, None) == -1
    for i in (0, 4, 6, 8, 9):                                                  # d_res_in (index 2) alone may be null
        args = [PTR, F32, None, 0, PTR, F32, PTR, F32, PTR, PTR, F32, 4, 256, None]
        args[i] = None
        assert b(*args) == -1
    assert b(PTR, F32, PTR, 5, PTR, F32, PTR, F32, PTR, PTR, F32, 4, 256, None) == -1       # a given d_res_in needs a valid dtype


def test_soft_att_depth_refuses(lib):
    f, b = lib.uenc_soft_att_depth_fwd, lib.uenc_soft_att_depth_bwd
    assert f(PTR, F32, PTR, PTR, 4, 72, None) == -1                             # D > 64
    assert f(PTR, F32, PTR, PTR, 4, 12, None) == -1                             # D % 8 != 0
    assert f(PTR, F32, PTR, PTR, 0, 32, None) == -1
    assert f(None, F32, PTR, PTR, 4, 32, None) == -1 and f(PTR, F32, None, PTR, 4, 32, None) == -1 and f(PTR, F32, PTR, None, 4, 32, None) == -1
    assert b(PTR, PTR, F32, PTR, PTR, F32, 4, 72, None) == -1
    assert b(PTR, PTR, F32, PTR, PTR, F32, 4, 20, None) == -1
    for i in (0, 1, 3, 4):
        args = [PTR, PTR, F32, PTR, PTR, F32, 4, 32, None]
        args[i] = None
        assert b(*args) == -1
    assert b(PTR, PTR, F32, PTR, PTR, 7, 4, 32, None) == -1


def test_wrappers_exist():
    from uenc import kernels as K
    for name in ("upsample2x_ac_fwd", "upsample2x_ac_bwd", "softmax_gate_fwd", "softmax_gate_bwd", "soft_att_depth_fwd", "soft_att_depth_bwd"):
        assert callable(getattr(K, name))
    assert ctypes.sizeof(ctypes.c_long) == 8
