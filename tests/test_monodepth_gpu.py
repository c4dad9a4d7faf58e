"""uenc_view_synth_* / uenc_photo_loss_* (csrc/monodepth.hip) and MonodepthLoss on the GPU against a float64 run of the module's torch path
on the fixture of tests/golden/monodepth_loss.npz."""
import numpy as np
import pytest
import torch

import monodepth_fixture as MF
from conftest import record_parity

pytestmark = pytest.mark.gpu

REL_L2 = 1e-4                   # the project's bar for fp32 kernels, as in tests/test_matcher_gpu.py
COMBOS = [(c, f) for c in MF.CASES for f in MF.FLAGSETS]


@pytest.fixture(scope="module")
def ML():
    import model  # noqa: F401  loads libuenc_hip.so
    import uenc.modeling.monodepth_loss as m
    return m


@pytest.fixture(scope="module")
def z():
    return MF.load()


@pytest.fixture(scope="module")
def ref64(ML, z):
    """The float64 torch path on the CPU, once per case and flag set."""
    return {(c, f): MF.run(ML.MonodepthLoss, z, c, f, dtype=torch.float64) for c, f in COMBOS}


@pytest.fixture(scope="module")
def measured(ML, z):
    """The kernel path, twice per case and flag set."""
    out = {}
    for c, f in COMBOS:
        out[(c, f)] = [MF.run(ML.MonodepthLoss, z, c, f, device="cuda", ctor_kwargs={"impl": "kernels"}) for _ in range(2)]
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case,flagset", COMBOS)
def test_kernel_path_matches_float64(ref64, measured, case, flagset):
    (losses, grads, outputs), _ = measured[(case, flagset)]
    l64, g64, o64 = ref64[(case, flagset)]
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
            figs[f"color/{f}/{s}"] = MF.rel_l2(outputs[("color", f, s)].detach().cpu().numpy(), o64[("color", f, s)].detach().numpy())
            figs[f"sample/{f}/{s}"] = MF.rel_l2(outputs[("sample", f, s)].detach().cpu().numpy(), o64[("sample", f, s)].detach().numpy())
    for k, e in figs.items():
        print(f"{case} {flagset} {k}: rel L2 {e:.3e}")
    record_parity(f"monodepth_vs_float64/{case}_{flagset}", **figs)
    for k, e in figs.items():
        assert e <= REL_L2, (k, e)


@pytest.mark.parametrize("case,flagset", COMBOS)
def test_two_runs_are_bit_identical(measured, case, flagset):
    (l1, g1, o1), (l2, g2, o2) = measured[(case, flagset)]
    assert torch.equal(l1["loss"], l2["loss"])
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for f in MF.FRAMES:
        for s in MF.SCALES:
            assert torch.equal(o1[("color", f, s)], o2[("color", f, s)])


@pytest.mark.parametrize("case,flagset", [(c, f) for c, f in COMBOS if MF.FLAGSETS[f]["bool_automask"]])
def test_argmin_maps_equal_the_restatement(ref64, measured, z, case, flagset):
    (_, _, outputs), _ = measured[(case, flagset)]
    _, _, o64 = ref64[(case, flagset)]
    same = 0
    for s in MF.SCALES:
        got = outputs[f"identity_selection/{s}"].cpu()
        assert torch.equal(got, o64[f"identity_selection/{s}"].float())
        assert np.array_equal(got.numpy().astype(np.uint8), z[f"{case}_{flagset}_idsel{s}"])       # and the reference's own
        same += got.numel()
    record_parity(f"monodepth_argmin/{case}_{flagset}", pixels_compared=same, differing=0)


def test_raw_argmin_without_automask(ML, z):
    """Two warped candidates only: the kernel's index equals torch.min's over the float64 per-candidate losses."""
    from uenc import kernels as K
    _, _, o64 = MF.run(ML.MonodepthLoss, z, "a", "rigid", dtype=torch.float64, backward=False)
    m = ML.MonodepthLoss(MF.make_cfg(*MF.CASES["a"]))
    target = torch.from_numpy(z["a_color0"]).double()
    color = torch.stack([torch.stack([o64[("color", f, s)].detach() for f in MF.FRAMES]) for s in MF.SCALES])
    _, arg = K.photo_loss_fwd(color.float().cuda().contiguous(), target.float().cuda())
    for s in MF.SCALES:
        want = torch.cat([m.compute_reprojection_loss(color[s, i], target) for i in range(2)], 1).argmin(1)
        assert torch.equal(arg[s].cpu().long(), want)


def test_loss_and_backward_replay_from_a_graph(ML, z):
    """generate_images_pred + compute_losses + backward recorded by torch.cuda.graph on one stream (any synchronisation or host read
    would fail the capture); the replay's loss and gradients equal the eager run's bit for bit."""
    case, flagset = "a", "full"
    B, H, W = MF.CASES[case]
    outputs, targets, leaves = MF.make_inputs(z, case, device="cuda")
    names = MF.leaf_names(flagset)
    noise = [torch.from_numpy(z[f"{case}_{flagset}_noise{s}"]).cuda() for s in MF.SCALES]
    ground = [torch.from_numpy(z[f"{case}_{flagset}_ground{s}"]).cuda() for s in MF.SCALES]
    m = ML.MonodepthLoss(MF.make_cfg(B, H, W, "cuda"), **MF.FLAGSETS[flagset], impl="kernels")
    base = dict(outputs)

    def step():
        o = dict(base)
        loss = m(o, targets, tie_noise=noise, ground_samples=ground)["loss_monodepth"]
        grads = torch.autograd.grad(loss, [leaves[n] for n in names])
        return loss.detach(), [g.detach() for g in grads]       # no reference to the autograd graph (and its leaf nodes) survives a step

    # every step runs on a side stream, the eager one too: a leaf's gradient node created on the default stream and still alive would make
    # the backward inside the capture synchronise with the default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager_loss, eager_grads = step()
        eager_loss, eager_grads = eager_loss.clone(), [g.clone() for g in eager_grads]
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grads = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, eager_loss)
    for n, a, b in zip(names, grads, eager_grads):
        assert torch.equal(a, b), n
    record_parity("monodepth_capture", replays=2, tensors_compared=len(names) + 1)
