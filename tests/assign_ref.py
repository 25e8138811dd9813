"""References of the max-IoU anchor assigner (csrc/assign.hip) for tests/test_assign_host.py and
tests/test_assign_gpu.py.

assign_from_iou: the rule, restated in numpy on a dense (G, N) IoU table of ONE frame -- no geometry, no window.
truth_table: float64 IoUs from targets_ref.poly_iou64 (bounding-circle pruning for speed only: circles that do not touch
hold boxes that do not touch, IoU exactly 0).
undecidable: where an f32 IoU within ``bound`` of the truth may decide differently from the truth."""
import numpy as np

import targets_ref as R


def assign_from_iou(iou, neg=0.45, pos=0.6, force=0.1):
    """iou (G, N), N anchors in flat order (x * W + y) * A + z.  Thresholds are compared in the table's own precision.
    Returns dict(pos (n_pos,) flat indices ascending, gi (n_pos,) the matched ground truth, notneg (n_neg,) ascending,
    gt_best (G,) = b(g), c (G,) = lowest anchor attaining b(g), forced (G,) bool: g holds an anchor by force)."""
    iou = np.asarray(iou)
    G, N = iou.shape
    t = iou.dtype.type
    empty = np.zeros((0,), np.int64)
    if G == 0 or N == 0:
        return dict(pos=empty, gi=empty, notneg=empty, gt_best=np.zeros((G,), iou.dtype), c=np.zeros((G,), np.int64),
                    forced=np.zeros((G,), bool))
    m, o = iou.max(axis=0), iou.argmax(axis=0)                     # argmax: the first = the lowest g
    b, c = iou.max(axis=1), iou.argmax(axis=1)                     # ... the lowest anchor
    is_pos = m >= t(pos)
    match = o.astype(np.int64)
    forced = np.zeros((G,), bool)
    if force <= 1.5:
        claim = {}
        for g in range(G):                                         # ascending g and a strict test: ties go to the lowest g
            if b[g] >= t(force) and (c[g] not in claim or iou[g, c[g]] > claim[c[g]][0]):
                claim[int(c[g])] = (iou[g, c[g]], g)
        for a, (_, g) in claim.items():                            # a forced match overrides o(a)
            is_pos[a] = True
            match[a] = g
            forced[g] = True
    notneg = (m >= t(neg)) | is_pos
    p = np.flatnonzero(is_pos)
    return dict(pos=p, gi=match[p], notneg=np.flatnonzero(notneg), gt_best=b, c=c.astype(np.int64), forced=forced)


def dense(res, n_anchors):
    """(positive (N,) bool, matched g (N,) i64 or -1, not negative (N,) bool) of an assign_from_iou result."""
    p = np.zeros((n_anchors,), bool)
    g = np.full((n_anchors,), -1, np.int64)
    nn = np.zeros((n_anchors,), bool)
    p[res['pos']] = True
    g[res['pos']] = res['gi']
    nn[res['notneg']] = True
    return p, g, nn


def triples(flat, W, A):
    flat = np.asarray(flat, np.int64)
    return [flat // (W * A), (flat // A) % W, flat % A]


def truth_table(gts, anchor_bevs):
    """gts (G,4,2), anchor_bevs (N,4,2) f32 -> (G, N) float64 IoUs."""
    gts = np.asarray(gts, np.float32).astype(np.float64).reshape(-1, 4, 2)
    an = np.asarray(anchor_bevs, np.float32).astype(np.float64).reshape(-1, 4, 2)
    out = np.zeros((gts.shape[0], an.shape[0]))
    ac = an.mean(axis=1)
    ar = np.sqrt(((an - ac[:, None]) ** 2).sum(axis=2)).max(axis=1)
    for g, q in enumerate(gts):
        gc = q.mean(axis=0)
        gr = np.sqrt(((q - gc) ** 2).sum(axis=1)).max()
        near = np.flatnonzero(np.sqrt(((ac - gc) ** 2).sum(axis=1)) <= gr + ar)
        for a in near:
            out[g, a] = R.poly_iou64(q, an[a])[1]
    return out


def _top2(x, axis):
    """Largest and second largest along ``axis`` (the second is -inf where there is only one entry)."""
    if x.shape[axis] < 2:
        first = x.max(axis=axis)
        return first, np.full(first.shape, -np.inf)
    s = np.sort(x, axis=axis)
    return np.take(s, -1, axis=axis), np.take(s, -2, axis=axis)


def undecidable(truth, neg, pos, force, bound):
    """(anchors (N,) bool, ground truths (G,) bool) where IoUs within ``bound`` of ``truth`` could decide differently.
    Anchors: m(a) within the bound of neg or pos; the two largest iou(., a) within twice the bound of each other and unequal, for
    an anchor at or near positive (by threshold, or a candidate best anchor of a box that may force).
    Ground truths: b(g) within the bound of force; the two largest iou(g, .) within twice the bound of each other.
    Which anchor an undecidable ground truth forces is then open as well: ``candidates`` names those anchors."""
    truth = np.asarray(truth, np.float64)
    G, N = truth.shape
    an, gt = np.zeros((N,), bool), np.zeros((G,), bool)
    if G == 0 or N == 0:
        return an, gt
    m, m2 = _top2(truth, 0)
    b, b2 = _top2(truth, 1)
    forcing = force <= 1.5
    may_force = forcing & (b >= force - bound)
    gt |= forcing & (np.abs(b - force) <= bound)
    gt |= may_force & (b - b2 <= 2 * bound)
    an |= (np.abs(m - neg) <= bound) | (np.abs(m - pos) <= bound)
    near_pos = (m >= pos - bound) | candidates(truth, may_force, bound)
    an |= near_pos & (m - m2 <= 2 * bound) & (m != m2)
    return an, gt


def candidates(truth, gts, bound):
    """(N,) bool: the anchors within twice the bound of the best IoU of one of the ground truths ``gts`` ((G,) bool) -- the ones
    an f32 table may pick as that box's best anchor."""
    truth = np.asarray(truth, np.float64)
    out = np.zeros((truth.shape[1],), bool)
    for g in np.flatnonzero(gts):
        out |= truth[g] >= truth[g].max() - 2 * bound
    return out
