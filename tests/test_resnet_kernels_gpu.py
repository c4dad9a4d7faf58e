"""The ResNet kernels (csrc/resnet.hip) through their `uenc.ops` / `uenc.kernels` entry points against float64 ATen on the host, computed
from the same fp32 inputs.  Figures are relative L2 errors unless a check is bit-for-bit; each is recorded (`record_parity("resnet_kernels/
...")`) before it is asserted.

Bars.  Stem convolution: the project's bars for an fp32 result (1e-4) and for one bf16 GEMM (1.5e-2) of tests/test_convnext_gpu.py; its
weight gradient 1e-3 in exact mode, where the fp32 GEMM has a fixed summation order and two calls must agree bit for bit (the product
mode's weight-gradient GEMM splits its rows over workgroups that add with float atomics: csrc/gemm.hip, not a kernel of this file).
Max pooling: the forward selects, so it equals ATen bit for bit; the backward adds at most 4 selected gradients per element in another
order than ATen, 1e-6.  In bf16 the upstream gradient is drawn from multiples of 1/8, so that those sums are exact and the comparison does
not hinge on where a bf16 rounding boundary falls.  The tie inputs relu(round(2 randn) / 2) must put a tie at the maximum of at least 30 %
of the windows.  For iid draws that share is 29 .. 31 % by the distribution itself (`tie_expectation`: 0.31 for a full 9-tap window, 0.29 for
the 4- and 6-tap windows at the border, 0 for the single tap of a 1 x 1 map), not far above 30 %, so the 30 % is asserted over the windows of
all five shapes together (30.4 %), and each shape is held to its own expectation: share >= expected - 4 sigma (sigma of a binomial over half
the windows, as neighbouring windows share a column), and at least that many tied windows, at least one wherever a tie can occur.  BatchNorm: statistics 1e-5, outputs 1e-4 (fp32) or
2^-9 + 1e-4 (bf16), gradients 1e-4 in exact mode, everything reproducible bit for bit.  The bf16 bar is taken element by element, as
tests/test_convnext_kernels_gpu.py takes it: a value rounded to nearest lies within half a unit in the last place, 2^-9 of the top of
its binade (up to 2^-8 of the value itself), of an fp32 value that meets the fp32 bar: |y - r64| <= 2^-9 * 2^(floor(log2 a) + 1) + bar with
a = |r64| + bar and bar = 1e-4 * max |r64|; a store that truncated misses it by a factor of up to 2.  The relative L2 bar 2^-9 + 1e-4 is
asserted as well on every map with at least 256 elements (correct rounding gives about 1.65e-3 there); on the 16-element map (1, 1, 2, 8)
the rounding alone lands at 2.1e-3 .. 2.7e-3 by chance, so there the element-wise bound stands alone and the L2 figure is recorded.  With x = 1000 + N(0, 1) a one-pass
E[x^2] - E[x]^2 in fp32 is off by about 6e-8 * 1e6 = 6e-2 in the variance, a stable form by about 1e-6: the 1e-4 bar separates them.
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import record_parity

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-5


def rel(a, b) -> float:
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def bf16_excess(y, r64) -> float:
    """max over elements of (|y - r64| - bar) / (top of the binade of |r64| + bar), bar = 1e-4 * max |r64|: <= 2^-9 for a bf16 value rounded to
    nearest from an fp32 value within bar of r64."""
    y, r = y.detach().double().cpu(), r64.detach().double().cpu()
    bar = 1e-4 * float(r.abs().max())
    top = torch.exp2(torch.floor(torch.log2(r.abs() + bar)) + 1)
    return float((((y - r).abs() - bar) / top).max())


L2_MIN_NUMEL = 256        # from here on the relative L2 of correct bf16 rounding (about 1.65e-3) is reliably below 2^-9 + 1e-4


def y_ok(y, r64, figs) -> bool:
    """fp32: relative L2 <= 1e-4.  bf16: relative L2 <= 2^-9 + 1e-4 on every map with at least L2_MIN_NUMEL elements, and the element-wise
    half-ulp bound (the docstring above) on every map, the 16-element one included, where the L2 figure of a correct kernel is a matter of
    chance."""
    if y.dtype == F32:
        return figs["y"] <= 1e-4
    figs["y_bf16_excess"] = bf16_excess(y, r64)
    return figs["y_bf16_excess"] <= 2.0 ** -9 and (y.numel() < L2_MIN_NUMEL or figs["y"] <= 2.0 ** -9 + 1e-4)


def tie_expectation(shape):
    """(expected share of windows whose maximum is tied, number of windows) for iid inputs relu(round(2 z) / 2), z ~ N(0, 1): a window with n
    taps inside the map ties unless exactly one tap holds the maximum, P = 1 - sum_v n P(v) P(< v)^(n - 1) over the values v = 0, 1/2, 1, ...
    (0.41, 0.32, 0.29, 0.29, 0.31 for n = 2, 3, 4, 6, 9; 0 for a single tap)."""
    import math
    Phi = lambda z: 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))
    pm = [Phi(0.25)] + [Phi((k + 0.5) / 2) - Phi((k - 0.5) / 2) for k in range(1, 40)]

    def p_tie(n):
        below, once = 0.0, 0.0
        for p in pm:
            once += n * p * below ** (n - 1) if n > 1 else p
            below += p
        return 1.0 - once
    B, H, W, C = shape
    taps = lambda o, L: sum(0 <= 2 * o + k - 1 < L for k in range(3))
    ps = [p_tie(taps(oy, H) * taps(ox, W)) for oy in range((H - 1) // 2 + 1) for ox in range((W - 1) // 2 + 1)]
    return sum(ps) / len(ps), B * C * len(ps)


def sid(s):
    return "x".join(map(str, s))


@pytest.fixture(scope="module")
def U():
    import model  # noqa: F401
    import uenc
    return uenc


@pytest.fixture()
def mode(request):
    from uenc import ops
    ops.set_exact(request.param == "exact")
    yield request.param
    ops.set_exact(False)


MODES = pytest.mark.parametrize("mode", ["exact", "bf16"], indirect=True)


def _randn(tag, shape):
    import zlib
    return torch.randn(shape, generator=torch.Generator().manual_seed(zlib.crc32(tag.encode())))


# ---- stem --------------------------------------------------------------------------------------------------------------------------
STEM_X = [(1, 3, 5, 6), (2, 3, 13, 18), (1, 3, 32, 41)]
_STEM = {}


def _stem_case(xs, Co):
    key = (xs, Co)
    if key not in _STEM:
        x, w = _randn("stem_x" + sid(xs), xs), _randn(f"stem_w{Co}", (Co, 3, 7, 7)) * (2.0 / 147) ** 0.5
        w64 = w.double().requires_grad_(True)
        y = F.conv2d(x.double(), w64, stride=2, padding=3)
        dy = _randn("stem_dy" + sid(tuple(y.shape)), tuple(y.shape))
        gw, = torch.autograd.grad(y, w64, dy.double())
        _STEM[key] = (x, w, dy, y.detach(), gw)
    return _STEM[key]


@MODES
@pytest.mark.parametrize("Co", [16, 64])
@pytest.mark.parametrize("xs", STEM_X, ids=sid)
def test_stem_conv(U, mode, xs, Co):
    from uenc import kernels as K, ops
    x, w, dy, y_ref, gw_ref = _stem_case(xs, Co)
    col = K.stem7x7_s2_patches(x.cuda())
    B, _, H, W = xs
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert col.shape == (B * Ho * Wo, 152) and col.dtype == K.adt() and tuple(y_ref.shape[2:]) == (Ho, Wo)
    # the patch matrix is pure data movement: (ky, kx, c) columns of the zero-padded image, 5 zero columns
    ref_col = F.unfold(x, 7, padding=3, stride=2).view(B, 3, 49, Ho * Wo).permute(0, 3, 2, 1).reshape(B * Ho * Wo, 147)
    assert torch.equal(col[:, :147].float().cpu(), ref_col.to(col.dtype).float()) and not bool(col[:, 147:].any())
    grads = []
    for _ in range(2):
        wp = w.clone().cuda().requires_grad_(True)
        y = ops.stem_conv7x7_s2(x.cuda(), wp)
        y.backward(dy.cuda().permute(0, 2, 3, 1).contiguous())
        torch.cuda.synchronize()
        grads.append(wp.grad.clone())
    figs = {"y": rel(y.permute(0, 3, 1, 2), y_ref), "dw": rel(grads[0], gw_ref), "dw_same_bits": float(torch.equal(grads[0], grads[1]))}
    print(figs)
    record_parity(f"resnet_kernels/stem_{mode}/{sid(xs)}_co{Co}", **figs)
    assert y.dtype == F32 and y.shape == (B, Ho, Wo, Co)
    assert figs["y"] <= (1e-4 if mode == "exact" else 1.5e-2)
    if mode == "exact":
        assert figs["dw"] <= 1e-3 and torch.equal(grads[0], grads[1])
    with pytest.raises(RuntimeError, match="no gradient for the image"):
        ops.stem_conv7x7_s2(x.cuda().requires_grad_(True), w.cuda())


# ---- max pooling -------------------------------------------------------------------------------------------------------------------
POOL = [(2, 7, 9, 16), (1, 12, 18, 40), (1, 2, 3, 8), (1, 1, 1, 64), (2, 23, 35, 16)]
_POOL = {}


def _pool_case(shape, dtype, ties):
    """Input, upstream gradient, and ATen's forward / backward on the host (fp32 arithmetic on the values the kernel sees)."""
    key = (shape, dtype, ties)
    if key not in _POOL:
        B, H, W, C = shape
        x = _randn(f"pool_x{ties}" + sid(shape), shape)
        if ties:
            x = torch.relu(torch.round(2 * x) / 2)
        x = x.to(dtype)
        xr = x.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        y = F.max_pool2d(xr, 3, 2, 1)
        dy = _randn("pool_dy" + sid(tuple(y.shape)), tuple(y.shape))
        if dtype == BF16:
            dy = torch.round(dy * 8) / 8
        y.backward(dy)
        win = F.unfold(F.pad(x.float().permute(0, 3, 1, 2), (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(B, C, 9, -1)
        tie_share = float(((win == win.amax(2, keepdim=True)).sum(2) > 1).float().mean())
        _POOL[key] = (x, dy.permute(0, 2, 3, 1).contiguous().to(dtype), y.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), tie_share)
    return _POOL[key]


@pytest.mark.parametrize("ties", [False, True], ids=["randn", "ties"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", POOL, ids=sid)
def test_max_pool(U, shape, dtype, ties):
    from uenc import ops
    x, dy, y_ref, dx_ref, tie_share = _pool_case(shape, dtype, ties)
    if ties:
        shares = [_pool_case(s, dtype, True)[4] for s in POOL]
        windows = [tie_expectation(s)[1] for s in POOL]
        pooled = sum(a * b for a, b in zip(shares, windows)) / sum(windows)
        assert pooled >= 0.30, (pooled, shares)
        expected, n = tie_expectation(shape)
        floor = max(0.0, expected - 4.0 * (expected * (1.0 - expected) / (n / 2)) ** 0.5)
        tied = round(tie_share * n)
        print({"tie_expected": expected, "tie_floor": floor, "tied_windows": tied})
        assert tie_share >= floor, (tie_share, floor)
        assert tied >= (max(1, int(floor * n)) if expected > 0 else 0), (tied, n)
    else:
        assert bool((y_ref < 0).any()) or shape[1] * shape[2] < 4          # some windows hold negative values only
    xi = x.cuda().requires_grad_(True)
    y = ops.max_pool3x3_s2(xi)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    figs = {"tie_share": tie_share, "y_equal": float(torch.equal(y.detach().float().cpu(), y_ref)), "dx": rel(xi.grad, dx_ref)}
    print(figs)
    record_parity(f"resnet_kernels/pool_{'ties' if ties else 'randn'}_{'f32' if dtype == F32 else 'bf16'}/{sid(shape)}", **figs)
    assert y.dtype == dtype and y.shape == y_ref.shape and xi.grad.dtype == dtype
    assert torch.equal(y.detach().float().cpu(), y_ref)
    assert figs["dx"] <= 1e-6


# ---- BatchNorm + residual + ReLU ---------------------------------------------------------------------------------------------------
BN = [(1, 1, 2, 8), (2, 3, 5, 16), (2, 23, 35, 16), (4, 16, 16, 40), (1, 7, 9, 264), (2, 64, 64, 64)]
_BN = {}


def _bn_inputs(shape):
    if shape not in _BN:
        C = shape[-1]
        t = {"x": _randn("bn_x" + sid(shape), shape) * 1.5 + 0.3, "res": _randn("bn_res" + sid(shape), shape), "dy": _randn("bn_dy" + sid(shape), shape),
             "gamma": torch.rand(C, generator=torch.Generator().manual_seed(C)) + 0.5, "beta": _randn(f"bn_beta{C}", (C,)) * 0.3,
             "rm": _randn(f"bn_rm{C}", (C,)) * 0.3, "rv": torch.rand(C, generator=torch.Generator().manual_seed(C + 1)) + 0.5}
        _BN[shape] = (t, {})
    return _BN[shape]


def _bn_ref(shape, train, res, relu):
    """float64 ATen on the host: F.batch_norm on the (M, C) rows + residual + ReLU, and autograd."""
    t, refs = _bn_inputs(shape)
    key = (train, res, relu)
    if key not in refs:
        C = shape[-1]
        d = {k: v.double() for k, v in t.items()}
        x, gamma, beta = (d[k].reshape(-1, C).requires_grad_(True) if k == "x" else d[k].requires_grad_(True) for k in ("x", "gamma", "beta"))
        r = d["res"].reshape(-1, C).requires_grad_(True)
        rm, rv = d["rm"].clone(), d["rv"].clone()
        y = F.batch_norm(x, rm, rv, gamma, beta, training=train, momentum=0.1, eps=EPS)
        if res:
            y = y + r
        if relu:
            y = torch.relu(y)
        gx, gg, gb, gr = torch.autograd.grad(y, [x, gamma, beta, r], d["dy"].reshape(-1, C), allow_unused=True)
        refs[key] = dict(y=y.detach(), dx=gx, dgamma=gg, dbeta=gb, dres=gr, rm=rm, rv=rv, mean=x.detach().mean(0), var=x.detach().var(0, unbiased=False))
    return t, refs[key]


def _bn_run(t, shape, train, res, relu, out_dtype, frozen=False):
    from uenc import kernels as K, ops
    C = shape[-1]
    c = {k: v.cuda() for k, v in t.items()}
    x = c["x"].reshape(-1, C).clone().requires_grad_(True)
    r = c["res"].reshape(-1, C).clone().requires_grad_(True) if res else None
    gamma, beta = c["gamma"].clone().requires_grad_(not frozen), c["beta"].clone().requires_grad_(not frozen)
    rm, rv, nbt = c["rm"].clone(), c["rv"].clone(), torch.zeros((), dtype=torch.int64, device="cuda")
    y = ops.bn_act(x, gamma, beta, rm, rv, nbt, residual=r, relu=relu, train=train, eps=EPS, out_dtype=out_dtype)
    y.backward(c["dy"].reshape(-1, C).to(y.dtype))
    torch.cuda.synchronize()
    mean, var = K.bn_stats(c["x"].reshape(-1, C)) if train else (rm, rv)
    return dict(y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, dres=None if r is None else r.grad, rm=rm, rv=rv, nbt=int(nbt),
                mean=mean, var=var)


@MODES
@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("shape", BN, ids=sid)
def test_bn_train(U, mode, shape, res, relu):
    from uenc import kernels as K
    t, ref = _bn_ref(shape, True, res, relu)
    out_dtype = F32 if mode == "exact" else BF16
    a = _bn_run(t, shape, True, res, relu, out_dtype)
    b = _bn_run(t, shape, True, res, relu, out_dtype)
    figs = {k: rel(a[k], ref[k]) for k in ("mean", "var", "y", "rm", "rv")}
    if mode == "exact":
        figs.update({k: rel(a[k], ref[k]) for k in ("dx", "dgamma", "dbeta")})
        if res:
            figs["dres"] = rel(a["dres"], ref["dres"])
    same = all(torch.equal(a[k], b[k]) for k in ("y", "dx", "dgamma", "dbeta", "mean", "var", "rm", "rv"))
    assert a["y"].dtype == K._odt(out_dtype) and a["nbt"] == 1
    assert figs["mean"] <= 1e-5 and figs["var"] <= 1e-5 and figs["rm"] <= 1e-5 and figs["rv"] <= 1e-5
    ok = y_ok(a["y"], ref["y"], figs)
    print(figs, same)
    record_parity(f"resnet_kernels/bn_train_{mode}/{sid(shape)}_{'res' if res else 'nores'}_{'relu' if relu else 'id'}", same_bits=float(same), **figs)
    assert ok, figs
    if mode == "exact":
        assert max(figs[k] for k in ("dx", "dgamma", "dbeta")) <= 1e-4 and figs.get("dres", 0.0) <= 1e-4
    assert same


def test_bn_train_bf16_out_in_fp32_arithmetic(U):
    """An fp32 input with a bf16 output (the maps inside a block in product mode)."""
    shape = (2, 23, 35, 16)
    t, ref = _bn_ref(shape, True, True, True)
    a = _bn_run(t, shape, True, True, True, BF16)
    figs = {"y": rel(a["y"], ref["y"])}
    ok = y_ok(a["y"], ref["y"], figs)
    record_parity("resnet_kernels/bn_train_bf16_out", **figs)
    assert a["y"].dtype == BF16 and ok, figs


def test_bn_stats_offset(U):
    from uenc import kernels as K
    shape = (2, 23, 35, 16)
    x = (1000.0 + _randn("bn_offset", shape)).reshape(-1, 16)
    mean, var = K.bn_stats(x.cuda())
    figs = {"mean": rel(mean, x.double().mean(0)), "var": rel(var, x.double().var(0, unbiased=False))}
    print(figs)
    record_parity("resnet_kernels/bn_stats_offset", **figs)
    assert figs["mean"] <= 1e-5 and figs["var"] <= 1e-4


@MODES
@pytest.mark.parametrize("frozen", [False, True], ids=["eval", "frozen"])
@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("shape", BN, ids=sid)
def test_bn_eval_and_frozen(U, mode, shape, res, relu, frozen):
    t, ref = _bn_ref(shape, False, res, relu)
    out_dtype = F32 if mode == "exact" else BF16
    a = _bn_run(t, shape, False, res, relu, out_dtype, frozen=frozen)
    b = _bn_run(t, shape, False, res, relu, out_dtype, frozen=frozen)
    figs = {"y": rel(a["y"], ref["y"])}
    keys = ["dx"] + ([] if frozen else ["dgamma", "dbeta"]) + (["dres"] if res else [])
    if mode == "exact":
        figs.update({k: rel(a[k], ref[k]) for k in keys})
    same = all(torch.equal(a[k], b[k]) for k in ["y"] + keys)
    ok = y_ok(a["y"], ref["y"], figs)
    print(figs, same)
    record_parity(f"resnet_kernels/bn_{'frozen' if frozen else 'eval'}_{mode}/{sid(shape)}_{'res' if res else 'nores'}_{'relu' if relu else 'id'}",
                  same_bits=float(same), **figs)
    assert a["nbt"] == 0 and torch.equal(a["rm"].cpu(), t["rm"]) and torch.equal(a["rv"].cpu(), t["rv"])      # running statistics untouched
    assert ok, figs
    if frozen:
        assert a["dgamma"] is None and a["dbeta"] is None
    if mode == "exact":
        assert max(figs[k] for k in keys) <= 1e-4
    assert same


def test_bn_refusals(U):
    from uenc import kernels as K, ops
    x = torch.randn(1, 8, device="cuda")
    v = torch.ones(8, device="cuda")
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.bn_act(x, v, v, v.clone(), v.clone(), None, train=True)
    assert ops.bn_act(x, v, v, v.clone(), v.clone(), None, train=False).shape == (1, 8)        # eval mode takes one row
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.bn_act(torch.randn(4, 12, device="cuda"), v, v, v, v, None)
    with pytest.raises(ValueError, match="multiple of 8"):
        K.maxpool3x3_s2_fwd(torch.randn(1, 4, 4, 12, device="cuda"))
