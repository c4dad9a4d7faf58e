"""The four entry points of csrc/monodepth.hip (`view_synth_fwd_kernel<0|1|2>`, `view_synth_bwd_pixel_kernel`, `view_synth_bwd_gather_kernel`,
`photo_loss_fwd_kernel`, `photo_loss_mean_kernel`, `photo_loss_bwd_kernel`) through `uenc_view_synth_fwd` / `_bwd` and `uenc_photo_loss_fwd` /
`_bwd` themselves, element by element against the float64 references of tests/monodepth_cases.py.

The C entry points are called directly with a 67-pointer descriptor filled here (as `uenc.kernels._vs_desc` fills it), so every buffer is the
test's own: outputs are prefilled with a sentinel NaN (no sentinel may survive, the guard elements behind each buffer must keep theirs), every
input is followed by NaN guards (a tap read past the end shows), and the workspaces are prefilled with NaN (stage B must read nothing stage A
did not write).  `uenc.kernels.view_synth_fwd` / `view_synth_bwd` / `photo_loss_fwd` / `photo_loss_bwd` run once each against the direct call,
bit for bit, and `MonodepthLoss` once in mode 1 (complete flow without the motion mask), which no flag set of tests/monodepth_fixture.py selects.

Bars (tests/monodepth_cases.py has the derivation; kappa = max(2 RHO32, 8) comes from fp32 torch on the CPU, never from a kernel):
  dense outputs   every element |kernel - r64| <= kappa 2^-24 M, M = max |r64| over the output's (scale, frame, image) item
  gT, p_photo     |kernel - r64| <= kappa 2^-24 A, A the float64 sum of the absolute per-pixel contributions
  argmin          equal wherever the two smallest float64 candidate values differ by more than twice the per-pixel value bar; everywhere in the
                  designed exact ties
  exact           two calls give the same bits; the gradient of a frame is exactly 0 wherever no window centre within one pixel selected it
No element is excused: the view-synthesis backward's discontinuities (floor, border clip) are kept out by zeros in the test's own gcolor at the
fragile pixels.  Each output's worst share of its bar is printed and recorded (`record_parity("monodepth_kernels/...")`) before anything is
asserted.  (B, H, W, S) = (1, 8, 66, 4) lies outside the contract (66 is no multiple of 2^(S - 1)): every entry point must refuse it.
"""
import math

import numpy as np
import pytest
import torch

import monodepth_cases as MC
import monodepth_fixture as MF
from conftest import record_parity
from test_monodepth_gpu import REL_L2          # the module-level bar of the whole-tensor tests

pytestmark = pytest.mark.gpu

SENT_BITS = 0x7FC0BEEF              # a NaN no kernel computes
SENT_U8 = 0xEE                      # no candidate index
GUARD = 64                          # elements behind every buffer
EINVAL = -1

# slots of struct VsDesc (csrc/monodepth.hip), restated: 67 pointers
SLOT = {"disp": 0, "cflow": 4, "mask": 12, "T": 20, "K": 21, "invK": 22, "src": 23, "color": 24, "sample": 25, "sample_ego": 26, "sample_cmp": 27,
        "depth": 28, "residual": 29, "gcolor": 37, "gres": 38, "gdisp": 46, "gcflow": 50, "gmask": 58, "gT": 66}


@pytest.fixture(scope="module")
def capi():
    from uenc import capi
    return capi


@pytest.fixture(scope="module")
def K():
    from uenc import kernels
    return kernels


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    record_parity("monodepth_kernels/rho32", **MC.RHO32)
    record_parity("monodepth_kernels/kappa", **MC.KAPPA)
    yield
    _REF.clear()
    MC._VS_INPUTS.clear()


class Out:
    """An output buffer: `shape` elements prefilled with the sentinel plus GUARD elements behind them."""

    def __init__(self, shape, u8=False):
        self.n, self.sent = int(np.prod(shape)), SENT_U8 if u8 else SENT_BITS
        self.raw = torch.full((self.n + GUARD,), self.sent, dtype=torch.uint8 if u8 else torch.int32, device="cuda")
        self.t = (self.raw[:self.n] if u8 else self.raw[:self.n].view(torch.float32)).view(shape)

    def ptr(self):
        return self.raw.data_ptr()

    def written(self):
        return not bool((self.raw[:self.n] == self.sent).any())

    def guard_intact(self):
        return bool((self.raw[self.n:] == self.sent).all())


def _in(a):
    """An fp32 input on the GPU with NaN guards behind it."""
    buf = torch.full((a.numel() + GUARD,), math.nan, device="cuda")
    buf[:a.numel()] = a.reshape(-1).cuda()
    return buf


def _workspace(n):
    """n floats of NaN with sentinel guards behind them."""
    o = Out((max(n, 1),))
    o.t.fill_(math.nan)
    return o


def _bits(a):
    return a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a


_REF = {}


def _vs_ref(run):
    """Inputs, conditions and r64 of a view-synthesis run: built once per module and left unchanged."""
    if ("vs", run) not in _REF:
        t, cond = MC.vs_inputs(run)
        _REF[("vs", run)] = (t, cond, MC.vs_reference(t, MC.VS_BY_ID[run[0]], run[1]))
    return _REF[("vs", run)]


def _ph_ref(cid):
    if ("ph", cid) not in _REF:
        case = MC.PH_BY_ID[cid]
        t = MC.ph_inputs(case)
        f64 = MC.ph_forward(t, case)
        maps = {w: MC.ph_argmin_map(case, w, f64["argmin"]) for w in MC.ph_maps(case)}
        _REF[("ph", cid)] = (t, f64, {w: (m, MC.ph_backward(t, case, m)) for w, m in maps.items()})
    return _REF[("ph", cid)]


def _vs_call(capi, case, mode, t):
    """uenc_view_synth_fwd and uenc_view_synth_bwd on buffers of the test's own -> (return codes, {name: Out or [Out]}, workspace)."""
    lib = capi.lib
    B, H, W, S, NF = (case[k] for k in ("B", "H", "W", "S", "NF"))
    d = np.zeros(67, dtype=np.uint64)
    keep = []

    def give(slot, a, i=0):
        keep.append(_in(a))
        d[SLOT[slot] + i] = keep[-1].data_ptr()

    for name, key in (("T", "T"), ("K", "K"), ("invK", "invK"), ("src", "src")):
        give(name, t[key])
    for s in range(S):
        give("disp", t["disp"][s], s)
    for i in range(S * NF):
        if mode >= 1:
            give("cflow", t["cflow"][i], i)
        if mode == 2:
            give("mask", t["mask"][i], i)
    o = dict(color=Out((S, NF, B, 3, H, W)), sample=Out((S, NF, B, H, W, 2)), depth=Out((S, B, 1, H, W)))
    if mode >= 1:
        o.update(sample_ego=Out((S, NF, B, H, W, 2)), sample_cmp=Out((S, NF, B, H, W, 2)), residual=[Out((B, 3, H, W)) for _ in range(S * NF)])
        for i, r in enumerate(o["residual"]):
            d[SLOT["residual"] + i] = r.ptr()
    for n in ("color", "sample", "depth") + (("sample_ego", "sample_cmp") if mode >= 1 else ()):
        d[SLOT[n]] = o[n].ptr()
    rc_f = lib.uenc_view_synth_fwd(d.ctypes.data, S, NF, B, H, W, mode, capi.stream_ptr())
    give("gcolor", t["gcolor"])
    for i, g in enumerate(t["gres"]):
        if mode >= 1 and g is not None:
            give("gres", g, i)
    o["gT"] = Out((NF, B, 4, 4))
    d[SLOT["gT"]] = o["gT"].ptr()
    o["gdisp"] = [Out((B, 1, H >> s, W >> s)) for s in range(S)]
    if mode >= 1:
        o["gcflow"] = [Out((B, 3, H >> (i // NF), W >> (i // NF))) for i in range(S * NF)]
    if mode == 2:
        o["gmask"] = [Out((B, 1, H >> (i // NF), W >> (i // NF))) for i in range(S * NF)]
    for n in ("gdisp", "gcflow", "gmask"):
        for i, b in enumerate(o.get(n, [])):
            d[SLOT[n] + i] = b.ptr()
    nws = lib.uenc_view_synth_workspace_floats(S, NF, B, H, W)
    ws = _workspace(nws)
    rc_b = lib.uenc_view_synth_bwd(d.ctypes.data, S, NF, B, H, W, mode, ws.ptr(), nws, capi.stream_ptr())
    torch.cuda.synchronize()
    return (rc_f, rc_b), o, ws, nws


def _outs(o):
    return [b for v in o.values() for b in (v if isinstance(v, list) else [v])]


def _value(name, o):
    """An output on the CPU in the reference's layout."""
    v = o[name]
    if name == "residual":
        return torch.stack([b.t for b in v]).cpu()
    return [b.t.cpu() for b in v] if isinstance(v, list) else v.t.cpu()


@pytest.mark.parametrize("run", MC.VS_RUNS, ids=MC.vs_run_id)
def test_view_synthesis_against_float64(capi, run):
    case, mode = MC.VS_BY_ID[run[0]], run[1]
    t, cond, r64 = _vs_ref(run)
    tag = f"monodepth_kernels/vs/{MC.vs_run_id(run)}"
    rc1, o1, ws1, nws = _vs_call(capi, case, mode, t)
    rc2, o2, ws2, _ = _vs_call(capi, case, mode, t)
    record_parity(f"{tag}/conditions", **cond)
    figs = {}
    for n in MC.vs_outputs(mode):
        got = _value(n, o1)
        share, err = MC.judge(n, got, r64[n], A=r64["A_gT"] if n == "gT" else None)
        figs[n] = dict(worst_share_of_bar=share, e_kernel=err, kappa=MC.KAPPA[n])
        print(f"{tag}/{n}", figs[n])
        record_parity(f"{tag}/{n}", **figs[n])
    assert rc1 == (0, 0) and rc2 == (0, 0), (rc1, rc2)
    assert nws == 5 * case["S"] * case["NF"] * case["B"] * case["H"] * case["W"] + case["S"] * case["NF"] * case["B"] * MC.vs_blocks(case) * 16
    assert set(o1) == set(MC.vs_outputs(mode))
    for b in _outs(o1) + _outs(o2):
        assert b.written() and b.guard_intact()                                # every element written, nothing behind the buffer
        assert bool(b.t.isfinite().all())                                      # with a workspace that held NaN
    assert ws1.guard_intact() and ws2.guard_intact()
    for n in MC.vs_outputs(mode):
        assert figs[n]["worst_share_of_bar"] <= 1.0, (MC.vs_run_id(run), n, figs[n])
    for a, b in zip(_outs(o1), _outs(o2)):                                     # two calls: the same bits (no atomics anywhere)
        assert torch.equal(_bits(a.t), _bits(b.t))


@pytest.mark.parametrize("c", MC.VS_REFUSED, ids=lambda c: c["id"])
def test_view_synthesis_refuses_a_width_the_scales_do_not_divide(capi, c):
    """W = 66 with four scales: 66 >> 3 = 8 columns would have to be upsampled by 8.25.  UENC_EINVAL from every entry point, nothing written."""
    lib = capi.lib
    case = dict(c, tscale=0.1, behind=False, seed=1)
    t = MC.vs_raw_inputs(case)
    assert lib.uenc_view_synth_workspace_floats(c["S"], c["NF"], c["B"], c["H"], c["W"]) == -1
    rc, o, _, _ = _vs_call(capi, case, 0, dict(t, gres=[None] * (c["S"] * c["NF"])))
    assert rc == (EINVAL, EINVAL)
    for b in _outs(o):
        assert not bool((b.raw != b.sent).any())
    assert lib.uenc_view_synth_workspace_floats(c["S"], c["NF"], c["B"], c["H"], 72) > 0      # the neighbouring width is accepted


def _ph_fwd(capi, case, g):
    lib = capi.lib
    S, NF, B, H, W = (case[k] for k in ("S", "NF", "B", "H", "W"))
    arg, p = Out((S, B, H, W), u8=True), Out((S,))
    nws = lib.uenc_photo_loss_workspace_floats(S, B, H, W)
    ws = _workspace(nws)
    rc = lib.uenc_photo_loss_fwd(g["color"].data_ptr(), g["target"].data_ptr(), g["src"].data_ptr() if case["automask"] else 0,
                                 g["noise"].data_ptr() if case["automask"] else 0, S, NF, B, H, W, case["automask"], ws.ptr(), nws, arg.ptr(),
                                 p.ptr(), capi.stream_ptr())
    torch.cuda.synchronize()
    return rc, arg, p, ws, nws


def _ph_bwd(capi, case, g, argmin):
    S, NF, B, H, W = (case[k] for k in ("S", "NF", "B", "H", "W"))
    gc = Out((S, NF, B, 3, H, W))
    am = torch.full((argmin.numel() + GUARD,), SENT_U8, dtype=torch.uint8, device="cuda")
    am[:argmin.numel()] = argmin.reshape(-1).cuda()
    rc = capi.lib.uenc_photo_loss_bwd(g["color"].data_ptr(), g["target"].data_ptr(), am.data_ptr(), g["gp"].data_ptr(), S, NF, B, H, W,
                                      case["automask"], gc.ptr(), capi.stream_ptr())
    torch.cuda.synchronize()
    return rc, gc


@pytest.mark.parametrize("cid", [c["id"] for c in MC.PH_CASES])
def test_photometric_loss_against_float64(capi, cid):
    case = MC.PH_BY_ID[cid]
    t, f64, maps = _ph_ref(cid)
    tag = f"monodepth_kernels/photo/{cid}"
    g = {n: _in(a) for n, a in t.items() if a is not None}
    tiles = MC.ph_tiles(case)
    rc1, arg1, p1, ws1, nws = _ph_fwd(capi, case, g)
    rc2, arg2, p2, ws2, _ = _ph_fwd(capi, case, g)
    tie = case["special"] in ("tie_warped", "tie_identity")
    judged = torch.ones_like(f64["argmin"], dtype=torch.bool) if tie else MC.judged_pixels(f64)
    share, err = MC.judge("p_photo", p1.t.cpu(), f64["p_photo"], A=f64["A"])
    differ = int(((arg1.t.cpu() != f64["argmin"]) & judged).sum())
    ffig = dict(worst_share_of_bar=share, e_kernel=err, kappa=MC.KAPPA["p_photo"], unjudged_share=1.0 - float(judged.double().mean()),
                judged_pixels_that_differ=differ, pixels_that_differ=int((arg1.t.cpu() != f64["argmin"]).sum()))
    print(f"{tag}/forward", ffig)
    record_parity(f"{tag}/forward", **ffig)
    bfig, grads = {}, {}
    for which, (m, g64) in maps.items():
        r1, gc1 = _ph_bwd(capi, case, g, m)
        r2, gc2 = _ph_bwd(capi, case, g, m)
        share, err = MC.judge("grad_color", gc1.t.cpu(), g64)
        bfig[which] = dict(worst_share_of_bar=share, e_kernel=err, kappa=MC.KAPPA["grad_color"])
        grads[which] = (r1, r2, gc1, gc2)
        print(f"{tag}/grad_color/{which}", bfig[which])
        record_parity(f"{tag}/grad_color/{which}", **bfig[which])
    assert rc1 == 0 and rc2 == 0 and nws == case["S"] * case["B"] * tiles[0] * tiles[1]
    for b in (arg1, p1, arg2, p2):
        assert b.written() and b.guard_intact()
    assert ws1.guard_intact() and bool(p1.t.isfinite().all())
    assert ffig["worst_share_of_bar"] <= 1.0, ffig
    assert differ == 0, ffig
    assert int(arg1.t.max()) < case["NF"] * (1 + case["automask"])
    assert torch.equal(arg1.t, arg2.t) and torch.equal(_bits(p1.t), _bits(p2.t))
    for which, (m, g64) in maps.items():
        r1, r2, gc1, gc2 = grads[which]
        assert r1 == 0 and r2 == 0
        assert gc1.written() and gc1.guard_intact() and bool(gc1.t.isfinite().all()), which
        assert bfig[which]["worst_share_of_bar"] <= 1.0, (cid, which, bfig[which])
        assert torch.equal(_bits(gc1.t), _bits(gc2.t)), which
        far = ~MC.selected_near(case, m).expand(-1, -1, -1, 3, -1, -1)
        assert not bool(gc1.t.cpu()[far].any()), which                          # exactly 0 where no window centre nearby selected the frame
        if which == "identity":
            assert not bool(gc1.t.any())


def test_wrappers_equal_the_direct_calls(capi, K):
    """uenc.kernels.view_synth_fwd / view_synth_bwd / photo_loss_fwd / photo_loss_bwd once each: the direct call's bits."""
    run = ("ragged-2blk", 2, "some")
    case = MC.VS_BY_ID[run[0]]
    t, _, _ = _vs_ref(run)
    rc, o, _, _ = _vs_call(capi, case, 2, t)
    assert rc == (0, 0)
    dev = lambda a: a.cuda().contiguous()
    args = (dev(t["K"]), dev(t["invK"]), dev(t["src"]), dev(t["T"]), [dev(a) for a in t["disp"]], [dev(a) for a in t["cflow"]],
            [dev(a) for a in t["mask"]])
    f = K.view_synth_fwd(2, *args)
    for n, m in (("color", "color"), ("sample", "sample"), ("depth", "depth"), ("sample_ego", "sample_ego"), ("sample_complete", "sample_cmp")):
        assert torch.equal(_bits(f[n]), _bits(o[m].t)), n
    for a, b in zip(f["residual"], o["residual"]):
        assert torch.equal(_bits(a), _bits(b.t))
    gT, gdisp, gcf, gmask = K.view_synth_bwd(2, *args, dev(t["gcolor"]), [None if g is None else dev(g) for g in t["gres"]])
    assert torch.equal(_bits(gT), _bits(o["gT"].t))
    for got, want in ((gdisp, o["gdisp"]), (gcf, o["gcflow"]), (gmask, o["gmask"])):
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert torch.equal(_bits(a), _bits(b.t))
    pc = MC.PH_BY_ID["one-tile"]
    pt, f64, _ = _ph_ref("one-tile")
    g = {n: _in(a) for n, a in pt.items()}
    rc, arg, p, _, _ = _ph_fwd(capi, pc, g)
    p2, arg2 = K.photo_loss_fwd(dev(pt["color"]), dev(pt["target"]), dev(pt["src"]), dev(pt["noise"]))
    assert rc == 0 and torch.equal(arg2, arg.t) and torch.equal(_bits(p2), _bits(p.t))
    rc, gc = _ph_bwd(capi, pc, g, f64["argmin"])
    gc2 = K.photo_loss_bwd(dev(pt["color"]), dev(pt["target"]), f64["argmin"].cuda(), dev(pt["gp"]), True)
    assert rc == 0 and torch.equal(_bits(gc2), _bits(gc.t))


def test_module_mode_1_matches_float64():
    """MonodepthLoss with the complete flow but without the motion mask (`view_synth_*_kernel<1>`: dX = dcf = dP, dres = gr only) on golden
    case a against the module's float64 torch path; the flags are passed directly, tests/monodepth_fixture.py has no such flag set."""
    import model  # noqa: F401  loads libuenc_hip.so
    from uenc.modeling.monodepth_loss import MonodepthLoss
    z = MF.load()
    B, H, W = MF.CASES["a"]
    names = [f"disp{s}" for s in MF.SCALES] + [f"T{f}" for f in MF.FRAMES] + [f"cflow{f}_{s}" for f in MF.FRAMES for s in MF.SCALES]

    def run(dtype, device, **kw):
        outputs, targets, leaves = MF.make_inputs(z, "a", dtype, device)
        m = MonodepthLoss(MF.make_cfg(B, H, W, device), bool_CmpFlow=True, bool_MotMask=False, **kw)
        m.generate_images_pred(outputs, targets)
        losses = m.compute_losses(targets, outputs)
        got = torch.autograd.grad(losses["loss"], [leaves[n] for n in names], allow_unused=True)
        return losses, {n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, got)}, outputs

    l64, g64, o64 = run(torch.float64, "cpu")
    losses, grads, outputs = run(torch.float32, "cuda", impl="kernels")
    figs = {}
    for k, v in l64.items():
        if k.startswith("loss_coef/"):
            assert float(losses[k]) == float(v)
            continue
        figs[k] = MF.rel_l2(MF.to_numpy(losses[k]), MF.to_numpy(v))
    for k, g in g64.items():
        figs["grad:" + k] = MF.rel_l2(grads[k].cpu().numpy(), g.numpy())
    for f in MF.FRAMES:
        for s in MF.SCALES:
            for n in ("color", "sample", "sample_ego", "sample_complete", "residual_flow"):
                figs[f"{n}/{f}/{s}"] = MF.rel_l2(outputs[(n, f, s)].detach().cpu().numpy(), o64[(n, f, s)].detach().numpy())
    for k, e in figs.items():
        print(f"module mode 1 {k}: rel L2 {e:.3e}")
    record_parity("monodepth_kernels/module_mode1", **figs)
    assert all(float(g64[f"cflow{f}_0"].abs().max()) > 0 for f in MF.FRAMES)          # the complete flow is reached
    for k, e in figs.items():
        assert e <= REL_L2, (k, e)
