"""The four entry points of csrc/criterion.hip, each against the float64 restatement of tests/criterion_cases.py on every case: point
logits, per-pair ce_n / dice_n, the full pred_masks gradient of every head, class loss and its gradient.  Each kernel runs twice and must
give the same bits."""
import pytest
import torch

from conftest import record_parity
from criterion_cases import CASES, EOS, build, counts, pairs_of, ref64, rel_l2

pytestmark = pytest.mark.gpu

REL_L2 = 1e-4                   # the project's bar for fp32 kernels, as in tests/test_matcher_gpu.py
WITH_PAIRS = [c for c in CASES if c != "H"]


@pytest.fixture(scope="module")
def K():
    import model  # noqa: F401  loads libuenc_hip.so
    from uenc import kernels
    return kernels


_DEV = {}


def device_case(K, name):
    """The case on the GPU: the call descriptor, flat index buffers and the float64 restatement's final points (heads * N, P, 2)."""
    if name not in _DEV:
        inp, ref = build(name), ref64(name)
        masks = [h["pred_masks"].cuda() for h in inp["heads"]]
        logits = [h["pred_logits"].cuda() for h in inp["heads"]]
        gts = [(t["masks"].view(torch.uint8) if t["masks"].dtype == torch.bool else t["masks"].to(torch.uint8)).cuda() for t in inp["targets"]]
        labels = [t["labels"].cuda() for t in inp["targets"]]
        d = {"call": K.CritCall(masks, logits, gts, labels), "row": None, "col": None}
        if inp["N"]:
            d["row"] = torch.cat([qi for head in inp["indices"] for qi, _ in head]).cuda()
            d["col"] = torch.cat([tj for head in inp["indices"] for _, tj in head]).cuda()
            d["points"] = torch.cat([r["points"] for r in ref]).cuda().contiguous()
        _DEV[name] = d
    return _DEV[name]


def max_abs(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


@pytest.mark.parametrize("name", [c for c in WITH_PAIRS if counts(c)[1]])
def test_point_logits(K, name):
    inp, ref, d = build(name), ref64(name), device_case(K, name)
    M = counts(name)[0]
    over = inp["draws"]["oversampled"].cuda().view(-1, M, 2)
    a = K.crit_point_logits(d["call"], d["row"], over)
    b = K.crit_point_logits(d["call"], d["row"], over)
    assert a.shape == (len(ref) * inp["N"], M) and torch.equal(a, b)
    want = torch.cat([r["point_logits"] for r in ref])
    e = rel_l2(a, want)
    print(f"{name}: point logits rel L2 {e:.3e}  max abs {max_abs(a, want):.3e}")
    record_parity(f"criterion_point_logits/{name}", rel_l2=e, max_abs=max_abs(a, want))
    assert e <= REL_L2
    # the selection the criterion makes from these logits is the float64 one, for every pair
    n_unc = counts(name)[1]
    keep = torch.topk(-a.abs(), n_unc, dim=1).indices.sort(dim=1).values.cpu()
    assert torch.equal(keep, torch.cat([r["keep"] for r in ref]))


@pytest.mark.parametrize("name", WITH_PAIRS)
def test_pair_losses(K, name):
    ref, d = ref64(name), device_case(K, name)
    a = K.crit_mask_loss_fwd(d["call"], d["row"], d["col"], d["points"], need_grad=True)
    b = K.crit_mask_loss_fwd(d["call"], d["row"], d["col"], d["points"], need_grad=True)
    c = K.crit_mask_loss_fwd(d["call"], d["row"], d["col"], d["points"], need_grad=False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and c[2] is None and c[3] is None
    ce, dice = torch.cat([r["ce"] for r in ref]), torch.cat([r["dice"] for r in ref])
    sums = torch.cat([torch.stack([(torch.sigmoid(r["x"]) * r["t"]).sum(1), torch.sigmoid(r["x"]).sum(1), r["t"].sum(1)], 1) for r in ref])
    figs = {"ce_rel_l2": rel_l2(a[0][:, 0], ce), "dice_rel_l2": rel_l2(a[0][:, 1], dice), "sums_rel_l2": rel_l2(a[1], sums),
            "ce_max_abs": max_abs(a[0][:, 0], ce), "dice_max_abs": max_abs(a[0][:, 1], dice)}
    print(name, figs)
    record_parity(f"criterion_pair_losses/{name}", **figs)
    assert figs["ce_rel_l2"] <= REL_L2 and figs["dice_rel_l2"] <= REL_L2 and figs["sums_rel_l2"] <= REL_L2
    # keys: every tap's cell, or h * w outside the map; case E must reach the sentinel
    h, w = CASES[name][3]
    keys = a[3]
    assert int(keys.min()) >= 0 and int(keys.max()) <= h * w
    if name == "E":
        assert int((keys == h * w).sum()) > 0


@pytest.mark.parametrize("name", WITH_PAIRS)
def test_mask_gradient(K, name):
    inp, ref, d = build(name), ref64(name), device_case(K, name)
    _, _, unit, keys = K.crit_mask_loss_fwd(d["call"], d["row"], d["col"], d["points"], need_grad=True)
    skeys, order = torch.sort(keys, dim=1, stable=True)
    gce, gdice = inp["coef"][:, 1].float().cuda().contiguous(), inp["coef"][:, 2].float().cuda().contiguous()
    args = (d["call"], d["row"], d["points"], unit, skeys, order, gce, gdice, 1.0 / inp["num_masks"])
    a = K.crit_mask_loss_bwd(*args)
    b = K.crit_mask_loss_bwd(*args)
    assert torch.equal(a, b)
    worst, worst_abs = 0.0, 0.0
    for i, r in enumerate(ref):
        worst, worst_abs = max(worst, rel_l2(a[i], r["g_masks"])), max(worst_abs, max_abs(a[i], r["g_masks"]))
        matched = torch.zeros(a.shape[1:3], dtype=torch.bool)
        for b_, q, _ in pairs_of(inp["indices"][i]):
            matched[b_, q] = True
        assert not a[i].cpu()[~matched].any()            # the maps of unmatched queries are exactly zero
        assert not r["g_masks"][~matched].any()
    print(f"{name}: pred_masks gradient rel L2 {worst:.3e}  max abs {worst_abs:.3e}")
    record_parity(f"criterion_mask_gradient/{name}", rel_l2=worst, max_abs=worst_abs)
    assert worst <= REL_L2


@pytest.mark.parametrize("name", list(CASES))
def test_class_loss(K, name):
    ref, d = ref64(name), device_case(K, name)
    a = K.crit_class_loss(d["call"], d["row"], d["col"], EOS)
    b = K.crit_class_loss(d["call"], d["row"], d["col"], EOS)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    want = torch.tensor([r["loss_ce"] for r in ref], dtype=torch.float64)
    grad = torch.stack([r["ce_grad_unit"] for r in ref]).reshape(len(ref), -1, CASES[name][2])
    figs = {"loss_rel_l2": rel_l2(a[0], want), "grad_rel_l2": rel_l2(a[1], grad), "loss_max_abs": max_abs(a[0], want), "grad_max_abs": max_abs(a[1], grad)}
    print(name, figs)
    record_parity(f"criterion_class_loss/{name}", **figs)
    assert figs["loss_rel_l2"] <= REL_L2 and figs["grad_rel_l2"] <= REL_L2


def test_argument_rejection(K):
    from uenc import capi
    d = device_case(K, "A")
    h = device_case(K, "H")
    with pytest.raises(capi.UencError):                  # no pairs: the mask entry points refuse, nothing is launched
        K.crit_mask_loss_fwd(h["call"], torch.zeros(0, dtype=torch.int64).cuda(), torch.zeros(0, dtype=torch.int64).cuda(),
                             torch.zeros(0, 16, 2).cuda())
    with pytest.raises(capi.UencError):
        K.crit_mask_loss_fwd(d["call"], d["row"].cpu(), d["col"], d["points"])
    with pytest.raises(capi.UencError):
        K.crit_point_logits(d["call"], d["row"], d["points"][:1])
    lib = capi.lib
    assert lib.uenc_crit_point_logits(None, 1, 1, 3, 5, 7, 2, 4, None, None, None, None) == -1
    assert lib.uenc_crit_mask_loss_fwd(None, 1, 1, 3, 5, 7, 20, 28, 2, 4, None, None, None, None, None, None, None, None) == -1
    assert lib.uenc_crit_mask_loss_bwd(None, 1, 1, 3, 5, 7, 2, 4, None, None, None, None, None, None, None, 1.0, None, None) == -1
    assert lib.uenc_crit_class_loss(None, 1, 1, 3, 4, 2, None, None, 0.1, None, None, None, None) == -1
    call = d["call"]
    assert lib.uenc_crit_point_logits(call.desc.ctypes.data, 1, 1, 3, 5, 7, 3, 4, d["row"].data_ptr(), d["points"].data_ptr(), d["points"].data_ptr(),
                                      None) == -1       # N that contradicts the descriptor's pair counts
    torch.cuda.synchronize()
