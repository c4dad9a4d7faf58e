"""The nearest-neighbour top-down merge of the plain FPN pixel decoders (csrc/fpn_nearest.hip) through `uenc_merge_nearest_tokens_fwd` /
`_bwd` and `ops.merge_nearest`, against F.interpolate(mode="nearest") + autograd on NCHW tensors.

  forward, fp32 output : a + nearest(prev) BIT-EQUAL to torch's fp32 `a + F.interpolate(prev, size, mode="nearest")` (one fp32 add per
                         element, the source index is ATen's); bf16 output: that sum rounded once, bit-equal to torch's `.bfloat16()`.
  adjoint              : dprev BIT-EQUAL to a float32 sum taken in the kernel's documented order -- the destination pixels of a source
                         pixel in row-major order (oy ascending, then ox ascending), accumulated one by one from 0.0f -- with the set
                         of destination pixels taken from torch's own forward (the index map F.interpolate gives an arange image); it
                         is also compared with the float64 autograd gradient within that order's rounding: n - 1 <= 14 additions
                         (the 1x1 -> 3x5 pair has the most destinations per source pixel, 15) of error <= 2^-24 each, relative
                         to the sum of magnitudes.
  bf16 dy              : the same order on the bf16 values widened to fp32.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
PAIRS = [((4, 7), (7, 13)), ((7, 13), (13, 25)), ((13, 25), (26, 50)), ((1, 1), (3, 5)), ((4, 7), (4, 7)), ((13, 25), (13, 25))]
CHANNELS = (32, 128)
B = 2


@pytest.fixture(scope="module")
def K():
    from uenc import kernels
    return kernels


def _data(src, dst, C, seed=0):
    g = torch.Generator().manual_seed(1000 * C + 10 * src[0] + dst[1] + seed)
    a = torch.randn(B, dst[0], dst[1], C, generator=g).cuda()
    prev = torch.randn(B, src[0], src[1], C, generator=g).cuda()
    dy = torch.randn(B, dst[0], dst[1], C, generator=g).cuda()
    return a, prev, dy


def _torch_forward(a, prev, dst):
    up = F.interpolate(prev.permute(0, 3, 1, 2), size=dst, mode="nearest").permute(0, 2, 3, 1)
    return a + up


def _index_map(src, dst):
    """(H, W) long: the flat source pixel torch's nearest resize reads for every destination pixel."""
    ar = torch.arange(src[0] * src[1], dtype=torch.float32, device="cuda").view(1, 1, *src)
    return F.interpolate(ar, size=dst, mode="nearest").view(*dst).long()


def _ordered_f32_sum(dy, src, dst):
    """dprev in float32, destination pixels added in row-major order one by one (the kernel's documented order)."""
    idx = _index_map(src, dst).view(-1)
    d = dy.float().view(B, dst[0] * dst[1], -1)
    acc = torch.zeros(B, src[0] * src[1], d.shape[-1], dtype=F32, device="cuda")
    rank = torch.zeros(src[0] * src[1], dtype=torch.long, device="cuda")
    order = []                                                   # rank of each destination pixel among its source pixel's, in row-major order
    for t in idx.tolist():
        order.append(int(rank[t])); rank[t] += 1
    order = torch.tensor(order, device="cuda")
    for r in range(int(order.max()) + 1):                        # round r adds every source pixel's r-th destination: one add each
        sel = (order == r).nonzero().view(-1)
        acc[:, idx[sel]] = acc[:, idx[sel]] + d[:, sel]
    return acc.view(B, src[0], src[1], -1)


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("src,dst", PAIRS, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in PAIRS])
def test_forward_is_torch_s_bit_for_bit(K, src, dst, C):
    a, prev, _ = _data(src, dst, C)
    want = _torch_forward(a, prev, dst)
    got = K.merge_nearest_tokens_fwd(a.view(B, -1, C), prev, dst, F32).view(B, *dst, C)
    assert got.dtype == F32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
    got16 = K.merge_nearest_tokens_fwd(a.view(B, -1, C), prev, dst, BF16).view(B, *dst, C)
    assert got16.dtype == BF16 and torch.equal(got16.view(torch.int16), want.bfloat16().view(torch.int16))
    # bf16 operands: widened, added in fp32
    a16, p16 = a.bfloat16(), prev.bfloat16()
    got = K.merge_nearest_tokens_fwd(a16.view(B, -1, C), p16, dst, F32).view(B, *dst, C)
    assert torch.equal(got.view(torch.int32), _torch_forward(a16.float(), p16.float(), dst).view(torch.int32))


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("src,dst", PAIRS, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in PAIRS])
def test_adjoint_is_the_ordered_float32_sum(K, src, dst, C):
    _, prev, dy = _data(src, dst, C)
    for d in (dy, dy.bfloat16()):
        got = K.merge_nearest_tokens_bwd(d.contiguous(), *src)
        assert got.dtype == F32 and got.shape == prev.shape
        want = _ordered_f32_sum(d, src, dst)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (src, dst, C, d.dtype)
        # and float64 autograd through F.interpolate: within the rounding of at most 14 ordered fp32 additions
        p64 = prev.double().requires_grad_(True)
        up = F.interpolate(p64.permute(0, 3, 1, 2), size=dst, mode="nearest").permute(0, 2, 3, 1)
        (g64,) = torch.autograd.grad(up, p64, d.double())
        up_abs = F.interpolate(p64.permute(0, 3, 1, 2), size=dst, mode="nearest").permute(0, 2, 3, 1)
        (gabs,) = torch.autograd.grad(up_abs, p64, d.double().abs())
        assert bool(((got.double() - g64).abs() <= 14 * 2.0 ** -24 * gabs).all()), (src, dst, C)


def test_every_source_pixel_is_reached_and_counts_add_up(K):
    """dy = 1: dprev counts the destinations of every source pixel -- all >= 1 when upsampling, their sum the destination size."""
    for src, dst in PAIRS:
        ones = torch.ones(B, *dst, 32, device="cuda")
        cnt = K.merge_nearest_tokens_bwd(ones, *src)
        assert bool((cnt >= 1).all()) and float(cnt[0, :, :, 0].sum()) == dst[0] * dst[1]


@pytest.mark.parametrize("out_dtype", [F32, BF16])
def test_autograd_node(out_dtype):
    """ops.merge_nearest: forward as above, gradient of `a` = dy, gradient of `prev` = the adjoint."""
    from uenc import ops
    src, dst, C = (7, 13), (13, 25), 128
    a, prev, dy = _data(src, dst, C, seed=5)
    at, pt = a.view(B, -1, C).clone().requires_grad_(True), prev.clone().requires_grad_(True)
    y = ops.merge_nearest(at, pt, dst, out_dtype=out_dtype)
    want = _torch_forward(a, prev, dst).view(B, -1, C)
    assert y.dtype == out_dtype and torch.equal(y.float(), want.to(out_dtype).float())
    da, dp = torch.autograd.grad(y, (at, pt), dy.view(B, -1, C).to(out_dtype))
    assert torch.equal(da, dy.view(B, -1, C).to(out_dtype).float())
    assert torch.equal(dp, _ordered_f32_sum(dy.to(out_dtype), src, dst))


REJECTS = [("C % 4 != 0", dict(C=6)), ("H = 0", dict(H=0)), ("Ws = 0", dict(Ws=0)), ("unknown dtype", dict(dtype=7)), ("misaligned", dict(off=4))]


@pytest.mark.parametrize("why,bad", REJECTS, ids=[w for w, _ in REJECTS])
def test_arguments_are_refused(why, bad):
    from uenc import capi
    a = dict(C=8, H=4, W=4, Hs=2, Ws=2, dtype=0, off=0)
    x = torch.ones(4096, device="cuda")
    out = torch.full((4096,), -7.0, device="cuda")
    call = lambda v: (capi.lib.uenc_merge_nearest_tokens_fwd(x.data_ptr() + v["off"], v["dtype"], x.data_ptr(), 0, out.data_ptr(), 0, 1, v["H"], v["W"],
                                                              v["Hs"], v["Ws"], v["C"], capi.stream_ptr()),
                      capi.lib.uenc_merge_nearest_tokens_bwd(x.data_ptr() + v["off"], v["dtype"], out.data_ptr(), 1, v["H"], v["W"], v["Hs"], v["Ws"],
                                                              v["C"], capi.stream_ptr()))
    assert call(dict(a, **bad)) == (-1, -1), why
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call(a) == (0, 0)
