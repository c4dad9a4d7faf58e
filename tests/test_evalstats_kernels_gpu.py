"""The three kernels of csrc/evalstats.hip against the numpy oracle of pq_cases.py: exact integer equality at the smallest shapes that
reach each branch (16-byte and one-pixel loads, LDS and global histogram, one and several chunks per workgroup, full and empty id
tables)."""
import numpy as np
import pytest
import torch

from pq_cases import LITERALS, numpy_confusion, numpy_pq_image, random_case
from targets_cases import colliding_ids

pytestmark = pytest.mark.gpu

S, DIM = 256, 258


@pytest.fixture(scope="module")
def K():
    from uenc import kernels
    return kernels


# ---- confusion matrix ------------------------------------------------------------------------------------------------------------------------
def _confusion(K, preds, gts, N, ignore, H, W, rs, max_blocks=0, conf=None):
    """preds[b]: (C, h, w) scores or (h, w) labels, gts[b]: (h, w), placed in one (B, H, W) batch whose padding holds valid labels and a
    clear class-0 winner, which must not be counted."""
    B, planar = len(preds), preds[0].ndim == 3
    gt = torch.from_numpy(rs.randint(0, N, (B, H, W)).astype(np.int32))
    if planar:
        pred = torch.zeros((B, preds[0].shape[0], H, W))
        pred[:, 0] = 7.0
    else:
        pred = torch.zeros((B, H, W), dtype=torch.int32)
    sizes = torch.zeros((B, 2), dtype=torch.int32)
    for b, (p, g) in enumerate(zip(preds, gts)):
        h, w = g.shape
        pred[b, ..., :h, :w] = torch.from_numpy(p)
        gt[b, :h, :w] = torch.from_numpy(g.astype(np.int32))
        sizes[b] = torch.tensor([h, w])
    if conf is None:
        conf = torch.zeros((N + 1, N + 1), dtype=torch.int64, device="cuda")
    K.eval_confusion(pred.cuda(), gt.cuda(), sizes.cuda(), conf, ignore, max_blocks)
    return conf


def _scores(rs, C, h, w):
    return rs.randint(0, 4, (C, h, w)).astype(np.float32)              # small integers: exact ties everywhere


def _truth(rs, N, ignore, h, w):
    g = rs.randint(-2, N + 3, (h, w))                                  # negative values and values >= N
    g[rs.rand(h, w) < 0.1] = ignore
    return g


@pytest.mark.parametrize("C,ignore", [(1, 255), (3, 1), (19, 255), (150, 255)])
def test_confusion_shapes_and_class_counts(K, C, ignore):
    """5 x 7 and 33 x 47 take one pixel per lane (H * W % 4 != 0), 96 x 160 16-byte loads over four chunks; C <= 63 counts in LDS, 150
    in global memory."""
    rs = np.random.RandomState(C)
    for h, w in ((5, 7), (33, 47), (96, 160)):
        p, g = _scores(rs, C, h, w), _truth(rs, C, ignore, h, w)
        conf = _confusion(K, [p], [g], C, ignore, h, w, rs).cpu().numpy()
        expect = numpy_confusion(p, g, C, ignore)
        assert conf.sum() == h * w and np.array_equal(conf, expect), (h, w)


@pytest.mark.parametrize("H,W", [(96, 160), (97, 161)])
@pytest.mark.parametrize("N", [19, 150])
def test_confusion_padded_batch_and_grid_stride(K, H, W, N):
    """Two images of different size in one padded batch; with one and two workgroups per image every workgroup takes several of the four
    chunks (the grid-stride loop)."""
    rs = np.random.RandomState(7)
    shapes = [(H, W), (50, 70)]
    preds = [_scores(rs, N, h, w) for h, w in shapes]
    gts = [_truth(rs, N, 255, h, w) for h, w in shapes]
    expect = sum(numpy_confusion(p, g, N, 255) for p, g in zip(preds, gts))
    for max_blocks in (0, 1, 2):
        conf = _confusion(K, preds, gts, N, 255, H, W, rs, max_blocks=max_blocks).cpu().numpy()
        assert np.array_equal(conf, expect), max_blocks


def test_confusion_ties_nan_label_map_and_accumulation(K):
    rs = np.random.RandomState(8)
    N, h, w = 6, 24, 40
    g = _truth(rs, N, 255, h, w)
    p = np.zeros((N, h, w), dtype=np.float32)                          # every plane equal: class 0 everywhere
    p[2, :, 10:] = p[5, :, 10:] = 3.0                                  # classes 2 and 5 tie for the maximum: 2
    p[4, :, 30:] = np.nan                                              # the first NaN wins, as torch.argmax has it
    p[5, :, 35:] = np.nan
    assert np.array_equal(torch.from_numpy(p).argmax(0).numpy(), np.argmax(p, axis=0))
    expect = numpy_confusion(p, g, N, 255)
    assert expect[0].sum() == 10 * h and expect[2].sum() == 20 * h and expect[4].sum() == 10 * h
    conf = _confusion(K, [p], [g], N, 255, h, w, rs)
    assert np.array_equal(conf.cpu().numpy(), expect)
    # a label map instead of scores (C == 0), labels outside [0, N) count in row N; accumulated into the same matrix
    lab = rs.randint(-1, N + 2, (h, w)).astype(np.int32)
    expect2 = numpy_confusion(lab, g, N, 255)
    assert expect2[N].sum() > 0
    _confusion(K, [lab], [g], N, 255, h, w, rs, conf=conf)
    assert np.array_equal(conf.cpu().numpy(), expect + expect2)
    _confusion(K, [p], [g], N, 255, h, w, rs, conf=conf)
    assert np.array_equal(conf.cpu().numpy(), 2 * expect + expect2)
    for shape in ((33, 47), (96, 160)):                                # two calls, same bytes: both load paths, both histograms
        for n in (19, 150):
            p, g = _scores(rs, n, *shape), _truth(rs, n, 255, *shape)
            a, b = (_confusion(K, [p], [g], n, 255, *shape, np.random.RandomState(1)).cpu() for _ in range(2))
            assert torch.equal(a, b)


# ---- panoptic quality ------------------------------------------------------------------------------------------------------------------------
def _expected_inter(pred, gt, gt_ids, pred_ids):
    def row(i, ids):
        if i == 0:
            return 0
        return ids.index(i) + 1 if i > 0 and i in ids else len(ids) + 1
    out = np.zeros((DIM, DIM), dtype=np.int64)
    pairs, counts = np.unique(np.stack([gt.reshape(-1), pred.reshape(-1)], axis=1), axis=0, return_counts=True)
    for (g, p), n in zip(pairs.tolist(), counts.tolist()):
        out[row(g, gt_ids), row(p, pred_ids)] += n
    return out


def _run_pq(K, cases, H, W, ncat, max_blocks=0, fill=0):
    """cases [(pred, pred_segs, gt, gt_segs)] in one padded (B, H, W) batch (padding = the id `fill` on both sides) -> inter, rec, fp, fn,
    unknown as numpy, and the raw device buffers."""
    B = len(cases)
    pred, gt = np.full((B, H, W), fill, dtype=np.int32), np.full((B, H, W), fill, dtype=np.int32)
    table = np.zeros(B * (5 * S + 4), dtype=np.int32)
    part = lambda k: table[k * B * S:(k + 1) * B * S].reshape(B, S)
    for b, (p, psegs, g, gsegs) in enumerate(cases):
        h, w = g.shape
        pred[b, :h, :w], gt[b, :h, :w] = p, g
        for k, col in ((0, 0), (2, 1), (3, 2)):
            part(k)[b, :len(gsegs)] = [s[col] for s in gsegs]
        for k, col in ((1, 0), (4, 1)):
            part(k)[b, :len(psegs)] = [s[col] for s in psegs]
        table[5 * B * S + b], table[5 * B * S + B + b] = len(gsegs), len(psegs)
        table[5 * B * S + 2 * B + 2 * b:5 * B * S + 2 * B + 2 * b + 2] = (h, w)
    table = torch.from_numpy(table).cuda()
    inter = K.eval_pq_intersect(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), table, max_blocks)
    out = K.eval_pq_match(inter, table, ncat)
    rec, fp, fn, unknown = (t.cpu().numpy() for t in K.eval_pq_unpack(out, B, ncat))
    return inter.cpu().numpy(), rec, fp, fn, unknown, (inter, out)


def _check_pq(K, cases, H, W, ncat, **kw):
    inter, rec, fp, fn, unknown, raw = _run_pq(K, cases, H, W, ncat, **kw)
    matches = 0
    for b, (p, psegs, g, gsegs) in enumerate(cases):
        assert np.array_equal(inter[b], _expected_inter(p, g, [s[0] for s in gsegs], [s[0] for s in psegs])), b
        e_rec, e_fp, e_fn, e_unknown = numpy_pq_image(p, psegs, g, gsegs, ncat)
        assert rec[b, :len(gsegs)].tolist() == [list(r) for r in e_rec], b
        assert (rec[b, len(gsegs):] == np.array([-1, 0, 0, -1])).all(), b
        assert fp[b].tolist() == e_fp.tolist() and fn[b].tolist() == e_fn.tolist() and unknown[b] == e_unknown, b
        matches += sum(r[0] >= 0 for r in e_rec)
    return matches, raw


def _full_table_case(rs, h, w, n_gt, n_pred, ncat):
    """Up to 256 ids that collide in the 9-bit hash on either side; every listed id has a pixel (the first rows hold them all, one pixel
    each), below that rectangles."""
    ids = colliding_ids(S)
    gt_ids, pred_ids = (ids[:n_gt] if n_gt != 1 else ids[200:201]), (ids[::-1][:n_pred] if n_pred != 1 else ids[7:8])
    pred, psegs, gt, gsegs = random_case(rs, h, w, gt_ids, pred_ids, ncat, crowd_every=9, unlisted_gt=2, rects=40)
    gt.reshape(-1)[:len(gt_ids)] = rs.permutation(np.array(gt_ids, dtype=np.int32))
    pred.reshape(-1)[:len(pred_ids)] = rs.permutation(np.array(pred_ids, dtype=np.int32))
    return pred, psegs, gt, gsegs


@pytest.mark.parametrize("h,w", [(32, 48), (31, 47)])
def test_pq_table_sizes_and_colliding_ids(K, h, w):
    """n_gt and n_pred in {0, 1, 256}, ids that share their low bits, id 0, ground-truth ids the table does not list (the unknown row)."""
    rs = np.random.RandomState(21)
    sizes = [(256, 256), (0, 1), (1, 0), (0, 0), (1, 256), (256, 1), (1, 1)]
    cases = [_full_table_case(rs, h, w, a, b, 19) for a, b in sizes]
    matches, _ = _check_pq(K, cases, h, w, 19)
    assert matches > 10


def test_pq_unknown_predictions_crowds_and_negative_ids(K):
    rs = np.random.RandomState(22)
    cases = [random_case(rs, 33, 47, range(1, 20), range(40, 60), 5, crowd_every=2, unlisted_gt=2, unlisted_pred=2),
             random_case(rs, 20, 31, [3, 3, 9, 0, -4, 12], [5, 6, 6, 0, 8], 5, crowd_every=3, unlisted_pred=1)]      # repeated and non-positive ids list nothing
    cases[1][0][2:4, 5:9] = -7
    cases[1][2][3:6, 6:11] = -4
    inter, rec, fp, fn, unknown, _ = _run_pq(K, cases, 33, 47, 5, fill=3)
    assert unknown[0] > 0 and unknown[1] > 0 and inter[0, :, 21].sum() == unknown[0]
    _check_pq(K, cases, 33, 47, 5, fill=3)


@pytest.mark.parametrize("case", LITERALS, ids=[c[0] for c in LITERALS])
def test_pq_rule_literals(K, case):
    _, images, _, ncat, _, counts = case
    _, rec, fp, fn, unknown, _ = _run_pq(K, images, 4, 4, ncat)
    tp = np.zeros(ncat, dtype=np.int64)
    for b, (_, _, _, gsegs) in enumerate(images):
        for col, inter, union, cat in rec[b, :len(gsegs)].tolist():
            tp[cat] += col >= 0
    assert {"tp": tp.tolist(), "fp": fp.sum(0).tolist(), "fn": fn.sum(0).tolist()} == counts and not unknown.any()
    _check_pq(K, images, 4, 4, ncat)
    if case[0] == "inside_same_class":
        assert rec[0, 0].tolist() == [0, 6, 8, 1]


@pytest.mark.parametrize("H,W", [(33, 47), (96, 160)])
def test_pq_random_maps_in_a_padded_batch(K, H, W):
    """Three images of different size in one padded batch whose padding holds a listed id; with one and two workgroups per image the
    96 x 160 maps (four chunks) go through the grid-stride loop; two calls give the same bytes."""
    rs = np.random.RandomState(23)
    ids = [1000 * (11 + k % 8) + k for k in range(30)] + [3, 4, 5]
    cases = [random_case(rs, H, W, ids, range(1, 34), 19), random_case(rs, H // 2, W - 5, ids[:10], range(1, 9), 19, crowd_every=2),
             random_case(rs, H - 1, W // 3, ids[5:25], range(50, 75), 19, unlisted_gt=0)]
    for max_blocks in (0, 1, 2):
        matches, (inter, out) = _check_pq(K, cases, H, W, 19, max_blocks=max_blocks, fill=ids[0])
        assert matches >= 5
        _, (inter2, out2) = _check_pq(K, cases, H, W, 19, max_blocks=max_blocks, fill=ids[0])
        assert torch.equal(inter, inter2) and torch.equal(out, out2)
