"""The cases of the set-criterion tests (tests/test_criterion_cpu.py, test_criterion_kernels_gpu.py, test_criterion_gpu.py): the case
table, seeded input builders with injected point draws and fixed indices, and a float64 restatement of the criterion's arithmetic.

What the restatement says, in this file's own words (nothing here imports the code under test):

  pairs      per head, the images in order, within an image the matched queries ascending: N = sum_b min(Q, T_b)
  sampling   a map (H, W) at a point (x, y) in [0, 1]^2: pixel coordinates x W - 1/2, y H - 1/2, the four surrounding cells weighted by
             (1 - |dx|)(1 - |dy|), cells outside the map count as zero.  The pixel coordinate is formed in fp32, ((2 p - 1 + 1) size - 1) / 2,
             because the points ARE fp32 numbers handed to an fp32 grid; everything after it (weights, sums, nonlinearities) is float64
  points     the n_unc = int(ratio P) oversampled points with the smallest |logit|, then the random ones
  ce_n       mean_p [max(x, 0) - x t + log(1 + exp(-|x|))];  dice_n = 1 - (2 sum s t + 1) / (sum s + sum t + 1), s = 1 / (1 + exp(-x))
  loss_mask  sum_n ce_n / num_masks, loss_dice likewise, num_masks = max(sum_b T_b, 1)
  loss_ce    sum w[y] (-log_softmax(logits)[y]) / sum w[y], y = the matched target's label or C (no object), w = 1, w[C] = eos_coef
Gradients come from float64 autograd through exactly these expressions.

Case validity: the GPU tests demand the IDENTICAL selected point set of every pair, which an fp32 kernel can only deliver when no
oversampled point sits at the selection threshold.  The builder therefore redraws oversampled points until, per pair, exactly n_unc of
them lie below a threshold by more than SEPARATION and all others above it by more than SEPARATION: the gap between the last kept and
the first dropped |logit| is then >= 2 * SEPARATION >= 1e-3 (test_criterion_cpu.py checks it in float64).
"""
import numpy as np
import torch

SEPARATION = 1e-3               # half the guaranteed |logit| gap at the selection threshold
MIN_GAP = 1e-3                  # what the issue asks of every pair
EOS = 0.1

#          bs  Q  C1  map       target      T per image  P     over  imp   heads  masks as
CASES = {
    "A":  (1, 3, 4, (5, 7), (20, 28), (2,), 100, 3.0, 0.75, 1, "bool"),          # P no multiple of a wave, odd map
    "B":  (2, 6, 5, (8, 12), (32, 48), (0, 4), 257, 3.0, 0.75, 3, "uint8"),      # an image without targets, several heads
    "C":  (1, 3, 4, (6, 9), (24, 36), (5,), 80, 3.0, 0.75, 2, "float"),          # more targets than queries, a repeated label
    "D1": (1, 2, 3, (1, 1), (4, 4), (2,), 300, 3.0, 0.75, 1, "bool"),            # every tap in one cell: the longest runs
    "D2": (2, 3, 3, (2, 3), (8, 12), (1, 2), 300, 3.0, 0.75, 2, "uint8"),
    "E":  (1, 4, 4, (6, 10), (24, 40), (3,), 64, 2.0, 0.5, 2, "uint8"),          # border points: dropped taps, sentinel keys
    "F":  (2, 150, 20, (32, 64), (128, 256), (19, 7), 12544, 3.0, 0.75, 10, "bool"),   # the configured point counts
    "G":  (1, 4, 4, (7, 9), (14, 18), (3,), 10, 2.5, 0.33, 2, "float"),          # int() truncation: M 25, 3 + 7
    "G0": (1, 4, 4, (7, 9), (14, 18), (3,), 10, 2.5, 0.0, 2, "float"),           # no top-k
    "G1": (1, 4, 4, (7, 9), (14, 18), (3,), 10, 2.5, 1.0, 2, "float"),           # no random tail
    "H":  (2, 4, 4, (5, 6), (10, 12), (0, 0), 16, 3.0, 0.75, 2, "uint8"),        # N = 0
}
SMALL = [c for c in CASES if c != "F"]
C_LABELS = (1, 1, 2, 0, 1)      # case C: a repeated label


def counts(name):
    P, over, imp = CASES[name][6:9]
    n_unc = int(imp * P)
    return int(P * over), n_unc, P - n_unc


def pairs_of(indices_head):
    """[(b, q, t), ...] of one head in pair order."""
    return [(b, int(q), int(t)) for b, (qi, tj) in enumerate(indices_head) for q, t in zip(qi.tolist(), tj.tolist())]


def pixel(p32, size):
    """The fp32 pixel coordinate of fp32 points, as a float64 tensor."""
    g = 2.0 * p32.float() - 1.0
    return (((g + 1.0) * float(size) - 1.0) / 2.0).double()


def bilinear64(maps, pts32):
    """maps (N, H, W) float64, pts32 (N, P, 2) fp32 x, y -> (N, P) float64."""
    N, H, W = maps.shape
    ix, iy = pixel(pts32[..., 0], W), pixel(pts32[..., 1], H)
    x0, y0 = ix.floor(), iy.floor()
    flat = maps.reshape(N, H * W)
    out = 0.0
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            wgt = (1 - (ix - xx).abs()) * (1 - (iy - yy).abs())
            inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            cell = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long()
            out = out + torch.where(inside, flat.gather(1, cell) * wgt, torch.zeros_like(wgt))
    return out


def border_points(h, w):
    """Case E: 0.0, the largest fp32 below 1, and points within half a pixel of each border of an (h, w) map."""
    big = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    nx, ny = 0.4 / w, 0.4 / h
    return torch.tensor([[0.0, 0.0], [big, big], [0.0, big], [big, 0.0], [nx, 0.5], [1 - nx, 0.5], [0.5, ny], [0.5, 1 - ny], [nx, 1 - ny],
                         [0.0, 0.5], [0.5, 0.0], [big, 0.5]], dtype=torch.float32)


def separate(src64, over, n_unc, n_fixed, gen):
    """Replaces oversampled points (never the first n_fixed of a pair) so that exactly n_unc per pair lie clearly below a threshold and
    the others clearly above it: the points too close to the threshold are exchanged for fresh draws from the side that lacks them."""
    N, M = over.shape[:2]
    free = torch.arange(M) >= n_fixed
    for n in range(N):
        mag = bilinear64(src64[n:n + 1], over[n:n + 1])[0].abs()
        thr = float(mag.kthvalue(n_unc).values + mag.kthvalue(n_unc + 1).values) / 2
        while n_fixed and bool(((mag[:n_fixed] - thr).abs() <= SEPARATION).any()):
            thr += 2 * SEPARATION
        below, above = mag < thr - SEPARATION, mag > thr + SEPARATION
        redo = ~(below | above)
        need_below = n_unc - int(below.sum())
        if need_below < 0:                               # only after the threshold moved for a fixed point
            redo[(below & free).nonzero()[:-need_below, 0]] = True
            need_below = 0
        need_above = int(redo.sum()) - need_below
        if need_above < 0:
            redo[(above & free).nonzero()[:-need_above, 0]] = True
            need_above = 0
        cand = torch.rand(8 * int(redo.sum()) + 64, 2, generator=gen)
        cmag = bilinear64(src64[n:n + 1], cand[None])[0].abs()
        lo, hi = cand[cmag < thr - SEPARATION], cand[cmag > thr + SEPARATION]
        assert lo.shape[0] >= need_below and hi.shape[0] >= need_above, "too few candidate points on one side of the threshold"
        over[n, redo] = torch.cat([lo[:need_below], hi[:need_above]])
    return over


_BUILT = {}


def build(name):
    """The inputs of a case (built once, never modified): outputs (fp32), targets, indices [head][image] -> (index_i, index_j) int64 on the
    CPU, draws {"oversampled", "random"}, coef (heads, 3) = the upstream gradient of each head's (loss_ce, loss_mask, loss_dice)."""
    if name in _BUILT:
        return _BUILT[name]
    bs, Q, C1, (h, w), (H, W), Ts, P, _, _, heads, mdt = CASES[name]
    M, n_unc, n_rnd = counts(name)
    gen = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    hd = [{"pred_logits": torch.randn(bs, Q, C1, generator=gen), "pred_masks": torch.randn(bs, Q, h, w, generator=gen) * 3} for _ in range(heads)]
    targets = []
    for T in Ts:
        m = torch.rand(T, H, W, generator=gen) > 0.5
        m = m if mdt == "bool" else m.to(torch.uint8) if mdt == "uint8" else m.float()
        labels = torch.tensor(C_LABELS[:T]) if name == "C" else torch.randint(0, C1 - 1, (T,), generator=gen)
        targets.append({"labels": labels.to(torch.int64), "masks": m})
    indices = []
    for _ in range(heads):
        per = []
        for T in Ts:
            k = min(Q, T)
            per.append((torch.randperm(Q, generator=gen)[:k].sort().values, torch.randperm(T, generator=gen)[:k]))
        indices.append(per)
    N = sum(min(Q, T) for T in Ts)
    over = torch.rand(heads, N, M, 2, generator=gen)
    rnd = torch.rand(heads, N, n_rnd, 2, generator=gen)
    n_fixed = 0
    if name == "E":
        bp = border_points(h, w)
        n_fixed = bp.shape[0]
        over[:, :, :n_fixed] = bp
        rnd[:, :, :n_fixed] = bp
    if N and n_unc:
        for i in range(heads):
            prs = pairs_of(indices[i])
            src = torch.stack([hd[i]["pred_masks"][b, q] for b, q, _ in prs]).double()
            over[i] = separate(src, over[i].clone(), n_unc, n_fixed, gen)
    coef = 0.5 + torch.rand(heads, 3, generator=gen, dtype=torch.float64)
    inp = {"name": name, "outputs": dict(hd[0], aux_outputs=hd[1:]), "heads": hd, "targets": targets, "indices": indices,
           "draws": {"oversampled": over, "random": rnd}, "coef": coef, "N": N, "num_classes": C1 - 1, "num_masks": float(max(sum(Ts), 1))}
    _BUILT[name] = inp
    return inp


def coef_dict(inp):
    """coef as a weight_dict-style mapping over the criterion's result keys."""
    out = {}
    for i in range(len(inp["heads"])):
        sfx = "" if i == 0 else f"_{i - 1}"
        for j, k in enumerate(("loss_ce", "loss_mask", "loss_dice")):
            out[k + sfx] = float(inp["coef"][i, j])
    return out


_REF = {}


def ref64(name):
    """The float64 restatement on a case -> per head a dict: point_logits (N, M), keep (N, n_unc) sorted indices of the selected
    oversampled points, gap (N,), points (N, P, 2) fp32, x / t (N, P), ce / dice (N,), loss_ce / loss_mask / loss_dice, target_classes,
    ce_grad_unit (the gradient of loss_ce alone), g_masks / g_logits (the gradients of sum_heads coef . losses).  Computed once."""
    if name in _REF:
        return _REF[name]
    inp = build(name)
    bs, Q, C1 = CASES[name][:3]
    M, n_unc, n_rnd = counts(name)
    N, nm = inp["N"], inp["num_masks"]
    res, total, leaves = [], 0.0, []
    for i, hd in enumerate(inp["heads"]):
        masks = hd["pred_masks"].double().requires_grad_(True)
        logits = hd["pred_logits"].double().requires_grad_(True)
        leaves.append((masks, logits))
        r = {}
        # class loss
        y = torch.full((bs, Q), C1 - 1, dtype=torch.int64)
        for b, q, t in pairs_of(inp["indices"][i]):
            y[b, q] = inp["targets"][b]["labels"][t]
        wv = torch.ones(C1, dtype=torch.float64)
        wv[C1 - 1] = EOS
        lsm = logits - logits.logsumexp(-1, keepdim=True)
        nll = -lsm.gather(-1, y[..., None])[..., 0]
        r["target_classes"] = y
        r["loss_ce"] = (wv[y] * nll).sum() / wv[y].sum()
        if N:
            prs = pairs_of(inp["indices"][i])
            src = torch.stack([masks[b, q] for b, q, _ in prs])
            tgt = torch.stack([inp["targets"][b]["masks"][t] for b, _, t in prs]).double()
            parts = []
            if n_unc:
                over = inp["draws"]["oversampled"][i]
                pl = bilinear64(src.detach(), over)
                order = pl.abs().argsort(dim=1, stable=True)
                srt = pl.abs().gather(1, order)
                r["point_logits"], r["keep"] = pl, order[:, :n_unc].sort(dim=1).values
                r["gap"] = srt[:, n_unc] - srt[:, n_unc - 1] if n_unc < M else torch.full((N,), float("inf"))
                parts.append(over.gather(1, order[:, :n_unc, None].expand(-1, -1, 2)))
            if n_rnd:
                parts.append(inp["draws"]["random"][i])
            pts = torch.cat(parts, dim=1)
            x, t = bilinear64(src, pts), bilinear64(tgt, pts)
            s = 1 / (1 + torch.exp(-x))
            ce = (x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).mean(1)
            dice = 1 - (2 * (s * t).sum(1) + 1) / (s.sum(1) + t.sum(1) + 1)
            r.update(points=pts, x=x.detach(), t=t, ce=ce.detach(), dice=dice.detach(), loss_mask=ce.sum() / nm, loss_dice=dice.sum() / nm)
        else:
            r.update(loss_mask=masks.sum() * 0, loss_dice=masks.sum() * 0)
        r["ce_grad_unit"] = torch.autograd.grad(r["loss_ce"], logits, retain_graph=True)[0]
        c = inp["coef"][i]
        total = total + c[0] * r["loss_ce"] + c[1] * r["loss_mask"] + c[2] * r["loss_dice"]
        res.append(r)
    total.backward()
    for r, (masks, logits) in zip(res, leaves):
        r["g_masks"], r["g_logits"] = masks.grad, logits.grad
        for k in ("loss_ce", "loss_mask", "loss_dice"):
            r[k] = float(r[k].detach())
    _REF[name] = res
    return res


def rel_l2(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu().reshape(-1), torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-300))


def final_points_sorted(points, n_unc):
    """The selected part of final points (N, P, 2) as a per-pair set: rows in lexicographic (x, y) order, so that two selections compare
    as sets."""
    sel = points[:, :n_unc].double()
    for c in (1, 0):                                     # stable sorts, the minor key first
        sel = sel.gather(1, sel[..., c].argsort(dim=1, stable=True)[..., None].expand(-1, -1, 2))
    return sel
