"""Shared by test_evaluators_cpu.py, test_evalstats_kernels_gpu.py and test_evaluators_gpu.py (no GPU needed here).

`numpy_pq` / `numpy_pq_image` and `numpy_confusion` are the ORACLE of the evaluators and of csrc/evalstats.hip: the third-party scorer
(panopticapi) is not installed, so its rules (uenc/evaluation.py's module docstring) are restated here on boolean masks, segment by
segment, without the intersection matrix that the product's host and device paths share.  LITERALS are worked by hand and come from
no code at all; `random_case` draws piecewise-constant maps of rectangles."""
import numpy as np

KEYS = ("PQ", "SQ", "RQ", "PQ_th", "SQ_th", "RQ_th", "PQ_st", "SQ_st", "RQ_st")


def numpy_confusion(pred, gt, num_classes, ignore_label):
    """conf[p, g] over the pixels; pred (C, H, W) scores (argmax, lowest index on a tie) or an (H, W) label map; a label outside
    [0, N), and a ground truth equal to ignore_label, count in row / column N."""
    pred, gt = np.asarray(pred), np.asarray(gt).astype(np.int64)
    lab = np.argmax(pred, axis=0) if pred.ndim == 3 else pred.astype(np.int64)
    N = num_classes
    lab = np.where((lab >= 0) & (lab < N), lab, N)
    gt = np.where((gt >= 0) & (gt < N) & (gt != ignore_label), gt, N)
    conf = np.zeros((N + 1, N + 1), dtype=np.int64)
    np.add.at(conf, (lab.reshape(-1), gt.reshape(-1)), 1)
    return conf


def _masks(m, ids):
    """One mask per listed id: an id <= 0 lists nothing, of two equal ids the first owns the pixels."""
    seen, out = set(), []
    for i in ids:
        out.append((m == i) if (i > 0 and i not in seen) else np.zeros(m.shape, dtype=bool))
        seen.add(i)
    return out


def numpy_pq_image(pred, pred_segs, gt, gt_segs, num_categories):
    """One image.  pred_segs [(id, category)], gt_segs [(id, category, iscrowd)] -> rec [(matched pred index or -1, inter, union, category)]
    per ground-truth segment, fp (K), fn (K), the pixel count of predicted ids that are neither 0 nor listed."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    void = gt == 0
    gm, pm = _masks(gt, [s[0] for s in gt_segs]), _masks(pred, [s[0] for s in pred_segs])
    ga, pa = [int(m.sum()) for m in gm], [int(m.sum()) for m in pm]
    rec, matched = [], set()
    for g, (_, gcat, crowd) in enumerate(gt_segs):
        row = (-1, 0, 0, gcat)
        if not crowd and ga[g]:
            for p, (_, pcat) in enumerate(pred_segs):
                if pcat != gcat or not pa[p]:
                    continue
                inter = int((gm[g] & pm[p]).sum())
                if inter == 0:
                    continue
                union = pa[p] + ga[g] - inter - int((void & pm[p]).sum())
                if inter / union > 0.5:
                    row = (p, inter, union, gcat)
                    matched.add(p)
        rec.append(row)
    fp, fn = np.zeros(num_categories, dtype=np.int64), np.zeros(num_categories, dtype=np.int64)
    for g, (_, gcat, crowd) in enumerate(gt_segs):
        if rec[g][0] < 0 and not crowd and ga[g] > 0:
            fn[gcat] += 1
    for p, (_, pcat) in enumerate(pred_segs):
        if p in matched:
            continue
        v = int((void & pm[p]).sum()) + sum(int((gm[g] & pm[p]).sum()) for g, (_, gcat, crowd) in enumerate(gt_segs) if crowd and gcat == pcat)
        if pa[p] and v / pa[p] > 0.5:
            continue
        fp[pcat] += 1
    listed = [i for i, _ in pred_segs if i > 0]
    unknown = int(((pred != 0) & ~np.isin(pred, listed)).sum())
    return rec, fp, fn, unknown


def numpy_pq(images, thing_ids, num_categories):
    """images = [(pred, pred_segs, gt, gt_segs), ...] -> (the nine figures times 100, {"tp", "fp", "fn"} per category)."""
    K = num_categories
    iou, tp, fp, fn = np.zeros(K), np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    for pred, pred_segs, gt, gt_segs in images:
        rec, f_p, f_n, unknown = numpy_pq_image(pred, pred_segs, gt, gt_segs, K)
        assert unknown == 0, "a predicted id that segments_info does not list"
        for col, inter, union, cat in rec:
            if col >= 0:
                tp[cat] += 1
                iou[cat] += inter / union
        fp += f_p
        fn += f_n
    out = {}
    for suffix, cats in (("", list(range(K))), ("_th", [c for c in range(K) if c in thing_ids]), ("_st", [c for c in range(K) if c not in thing_ids])):
        rows = [(iou[c] / (tp[c] + fp[c] / 2 + fn[c] / 2), iou[c] / tp[c] if tp[c] else 0.0, tp[c] / (tp[c] + fp[c] / 2 + fn[c] / 2))
                for c in cats if tp[c] + fp[c] + fn[c] > 0]
        for k, name in enumerate(("PQ", "SQ", "RQ")):
            out[name + suffix] = 100 * sum(r[k] for r in rows) / len(rows) if rows else 0.0
    return out, {"tp": tp.tolist(), "fp": fp.tolist(), "fn": fn.tolist()}


# ---- literals, worked by hand ---------------------------------------------------------------------------------------------------------------
def _grid(rows):
    return np.array([[int(ch) for ch in r] for r in rows], dtype=np.int32)


def _res(all3, th3, st3):
    return dict(zip(KEYS, tuple(all3) + tuple(th3) + tuple(st3)))


_GT8 = _grid(["5555", "5555", "0000", "0000"])                      # one ground-truth segment (id 5) of 8 pixels, the rest VOID
_IN6 = _grid(["3330", "3330", "0000", "0000"])                      # a prediction (id 3) of 6 pixels inside it
_HALF = _grid(["0000", "3333", "3333", "0000"])                     # 8 pixels: 4 over the segment, 4 over VOID
_MORE = _grid(["0000", "0333", "3333", "3000"])                     # 8 pixels: 3 over the segment, 5 over VOID
_GT_CROWD = _grid(["7777", "7777", "0055", "0055"])                 # a crowd (id 7) of 8 pixels, a segment (id 5) of 4
_PR_CROWD = _grid(["3330", "3330", "0044", "0044"])                 # 6 pixels inside the crowd; the segment predicted exactly (id 4)
_GT_STUFF = _grid(["6600", "6600", "0000", "0000"])
_PR_STUFF = _grid(["2200", "2200", "0000", "0000"])
Z = (0.0, 0.0, 0.0)

# name, images [(pred, [(id, cat)], gt, [(id, cat, crowd)])], thing ids, K, expected figures, expected tp / fp / fn per category
LITERALS = [
    # inter 6, union 6 + 8 - 6 - 0 = 8: IoU 0.75 > 0.5, a TP of category 1; categories 0 and 2 are never seen and stay out of the mean
    ("inside_same_class", [(_IN6, [(3, 1)], _GT8, [(5, 1, 0)])], [1, 2], 3, _res((75.0, 75.0, 100.0), (75.0, 75.0, 100.0), Z),
     {"tp": [0, 1, 0], "fp": [0, 0, 0], "fn": [0, 0, 0]}),
    # the categories differ: no pair; the prediction (nothing of it over VOID) is an FP of 2, the segment an FN of 1
    ("inside_other_class", [(_IN6, [(3, 2)], _GT8, [(5, 1, 0)])], [1, 2], 3, _res(Z, Z, Z),
     {"tp": [0, 0, 0], "fp": [0, 0, 1], "fn": [0, 1, 0]}),
    # inter 4, union 8 + 8 - 4 - 4 = 8: IoU 0.5 is no match; 4 of 8 pixels over VOID is not MORE than half: counted as FP
    ("half_over_void", [(_HALF, [(3, 1)], _GT8, [(5, 1, 0)])], [1, 2], 3, _res(Z, Z, Z),
     {"tp": [0, 0, 0], "fp": [0, 1, 0], "fn": [0, 1, 0]}),
    # one pixel more over VOID (5 of 8): the prediction is skipped, only the FN stays
    ("more_than_half_over_void", [(_MORE, [(3, 1)], _GT8, [(5, 1, 0)])], [1, 2], 3, _res(Z, Z, Z),
     {"tp": [0, 0, 0], "fp": [0, 0, 0], "fn": [0, 1, 0]}),
    # the crowd (category 1) absorbs the prediction of its own class (6 of 6 pixels) and adds no FN; the other pair is IoU 1 in category 2
    ("crowd_absorbs_own_class", [(_PR_CROWD, [(3, 1), (4, 2)], _GT_CROWD, [(7, 1, 1), (5, 2, 0)])], [1, 2], 3,
     _res((100.0, 100.0, 100.0), (100.0, 100.0, 100.0), Z), {"tp": [0, 0, 1], "fp": [0, 0, 0], "fn": [0, 0, 0]}),
    # the same prediction with category 0 is not the crowd's class: an FP of 0 (stuff); All = mean of categories 0 and 2
    ("crowd_other_class", [(_PR_CROWD, [(3, 0), (4, 2)], _GT_CROWD, [(7, 1, 1), (5, 2, 0)])], [1, 2], 3,
     _res((50.0, 50.0, 50.0), (100.0, 100.0, 100.0), Z), {"tp": [0, 0, 1], "fp": [1, 0, 0], "fn": [0, 0, 0]}),
    # two images, K = 4: category 1 has IoU 0.75, category 0 (stuff) IoU 1; categories 2 and 3 are never seen: All = (75 + 100) / 2
    ("unseen_categories_excluded", [(_IN6, [(3, 1)], _GT8, [(5, 1, 0)]), (_PR_STUFF, [(2, 0)], _GT_STUFF, [(6, 0, 0)])], [1, 2], 4,
     _res((87.5, 87.5, 100.0), (75.0, 75.0, 100.0), (100.0, 100.0, 100.0)), {"tp": [1, 1, 0, 0], "fp": [0, 0, 0, 0], "fn": [0, 0, 0, 0]}),
]


# ---- random piecewise-constant maps --------------------------------------------------------------------------------------------------------
def _paint(rs, m, ids, count):
    h, w = m.shape
    for _ in range(count):
        y0, x0 = rs.randint(0, h), rs.randint(0, w)
        m[y0:y0 + rs.randint(1, max(2, h // 2)), x0:x0 + rs.randint(1, max(2, w // 2))] = ids[rs.randint(0, len(ids))]


def random_case(rs, h, w, gt_ids, pred_ids, num_categories, crowd_every=5, unlisted_gt=1, unlisted_pred=0, rects=24):
    """-> (pred, pred_segs, gt, gt_segs): the ground truth is rectangles of gt_ids, VOID and `unlisted_gt` ids its table does not list; the
    prediction repeats it under its own ids (the k-th predicted id for the k-th ground-truth id, mostly of the same category, so that
    pairs match) and is then painted over with further rectangles of pred_ids, 0 and `unlisted_pred` unlisted ids."""
    gt_ids, pred_ids = [int(i) for i in gt_ids], [int(i) for i in pred_ids]
    top = max(gt_ids + pred_ids + [0])
    gt = np.zeros((h, w), dtype=np.int32)
    _paint(rs, gt, gt_ids + [0] + [top + 1 + k for k in range(unlisted_gt)], rects)
    pred = np.zeros((h, w), dtype=np.int32)
    for k in range(min(len(gt_ids), len(pred_ids))):
        pred[gt == gt_ids[k]] = pred_ids[k]
    _paint(rs, pred, pred_ids + [0] + [top + 100 + k for k in range(unlisted_pred)], rects // 3)
    gt_segs = [(i, int(rs.randint(0, num_categories)), int(bool(crowd_every) and k % crowd_every == crowd_every - 1)) for k, i in enumerate(gt_ids)]
    pred_segs = [(i, gt_segs[k][1] if k < len(gt_segs) and rs.rand() < 0.8 else int(rs.randint(0, num_categories))) for k, i in enumerate(pred_ids)]
    return pred, pred_segs, gt, gt_segs


def infos(segs):
    """(id, category[, iscrowd]) rows -> segments_info dicts."""
    return [dict(zip(("id", "category_id", "iscrowd"), (int(v) for v in s))) for s in segs]
