"""Inputs of the test-time augmentation's fusion tests (tests/test_tta_host.py, tests/test_tta_gpu.py): planted ground boxes
seen in V views -- each view's list is the planted boxes through ``Geometry.transform_boxes`` of its row plus a small jitter,
with distinct scores, sorted and padded as ``postprocess(read=False)`` leaves it.

The decisions are well conditioned by construction and ``build`` asserts it on the CPU, with the reference alone: every
pairwise IoU of a merged list lies at least ``MARGIN`` away from ``iou_thr`` and from ``fuse_iou``, merged scores are distinct
or exact ties (decided by view, then rank), fused scores are distinct."""
import math

import numpy as np

import tta_ref as R

MARGIN = 1e-3
IOU_THR, FUSE_IOU = 0.1, 0.5
VIEWS3 = np.array([[0.0, 1.0, 0.0, 0.0], [0.3, 1.05, 1.0, 0.0], [-0.2, 0.95, 0.0, 0.0]], np.float32)


def _transform(boxes, row):
    from modules.augment.Geometry import transform_boxes
    return transform_boxes(np.asarray(boxes, np.float32), row)


def planted(n, seed):
    """n car-sized boxes on an 8 m x 12 m lattice (no two touch, whatever their yaws), yaws over the full turn; the first
    four sit at the +-pi seam."""
    g = np.random.default_rng(seed)
    b = np.zeros((n, 7))
    for k in range(n):
        b[k, 0] = 8.0 + 8.0 * (k % 8) + g.uniform(-0.5, 0.5)
        b[k, 1] = -24.0 + 12.0 * (k // 8) + g.uniform(-0.5, 0.5)
    b[:, 2] = g.uniform(-1.8, -0.6, n)
    b[:, 3] = g.uniform(3.6, 4.4, n)
    b[:, 4] = g.uniform(1.5, 1.8, n)
    b[:, 5] = g.uniform(1.4, 1.7, n)
    b[:, 6] = g.uniform(-math.pi, math.pi, n)
    b[:4, 6] = [3.135, -3.135, 3.14, -3.14]
    return b.astype(np.float32)


def _pack(per_view, post_max):
    """Per view a list of (box7, score) -> (boxes (V, post_max, 7), scores (V, post_max), counts (V,)), score descending."""
    V = len(per_view)
    boxes = np.zeros((V, post_max, 7), np.float32)
    scores = np.zeros((V, post_max), np.float32)
    counts = np.zeros((V,), np.int32)
    for v, items in enumerate(per_view):
        items = sorted(items, key=lambda t: -t[1])
        assert len(items) <= post_max
        for k, (b, s) in enumerate(items):
            boxes[v, k], scores[v, k] = b, s
        counts[v] = len(items)
    return boxes, scores, counts


def _frame(ground, views, post_max, g, empty_view=None):
    """One source frame's lists.  Ground box 0 is seen twice in view 0 (two would-be voters of one view), box 1 in view 1
    only (a cluster of a single view), box 2 has a last-view sighting 2 m along its length off (IoU between the two thresholds:
    a member that does not vote); everything else once per view with a jitter of a few centimetres and 0.02 rad."""
    V = views.shape[0]
    per_view = [[] for _ in range(V)]
    pool = list(np.round(g.permutation(900)[:V * post_max + 8] / 1000.0 + 0.05, 3).astype(np.float32))      # distinct scores
    for k, gb in enumerate(ground):
        for v in range(V):
            if v == empty_view or (k == 1 and v != 1 % V):
                continue
            b = gb.astype(np.float64).copy()
            b[:2] += g.uniform(-0.05, 0.05, 2)
            b[2] += g.uniform(-0.03, 0.03)
            b[3:6] *= g.uniform(0.98, 1.02, 3)
            b[6] += g.uniform(-0.02, 0.02)
            if k == 2 and v == V - 1:
                b[0] += 2.0 * math.cos(b[6])
                b[1] -= 2.0 * math.sin(b[6])
            per_view[v].append((_transform(b[None], views[v])[0], pool.pop()))
            if k == 0 and v == 0:
                b2 = b.copy()
                b2[:2] += [0.04, -0.03]
                per_view[v].append((_transform(b2[None], views[v])[0], pool.pop()))
    return per_view, pool


def build(seed=0, post_max=24, n_ground=(22, 9), views=VIEWS3):
    """F = len(n_ground) source frames x V views: dict(boxes (F*V, post_max, 7), scores, counts, views, F, ground).  The last
    frame's last view is empty.  Two exact score ties are planted across views of frame 0."""
    g = np.random.default_rng(seed)
    V, F = views.shape[0], len(n_ground)
    boxes, scores, counts, ground = [], [], [], []
    for f, n in enumerate(n_ground):
        gb = planted(n, seed + 10 * f)
        per_view, _ = _frame(gb, views, post_max, g, empty_view=V - 1 if f == F - 1 and F > 1 else None)
        if f == 0 and V > 1 and n >= 12:        # exact ties across views: (view, rank) decides
            per_view[1][3] = (per_view[1][3][0], per_view[0][5][1])
            per_view[V - 1][7] = (per_view[V - 1][7][0], per_view[0][9][1])
        b, s, c = _pack(per_view, post_max)
        boxes.append(b); scores.append(s); counts.append(c); ground.append(gb)
    case = dict(boxes=np.concatenate(boxes), scores=np.concatenate(scores), counts=np.concatenate(counts), views=views, F=F,
                ground=ground, post_max=post_max)
    check_margins(case)
    return case


def check_margins(case, iou_thr=IOU_THR, fuse_iou=FUSE_IOU):
    """The conditions the exact comparisons rest on, from the reference alone."""
    out = R.fuse(case['boxes'], case['scores'], case['counts'], case['views'], case['F'], iou_thr, fuse_iou)
    for fr in out:
        iou = fr['iou']
        n = iou.shape[0]
        upper = iou[np.triu_indices(n, 1)]
        assert (np.abs(upper - iou_thr) >= MARGIN).all() and (np.abs(upper - fuse_iou) >= MARGIN).all()
        ms, prov = fr['merged'][1], fr['merged'][2]
        for i in range(n - 1):                  # merged order is strict: score, then view * post_max + rank
            assert ms[i] > ms[i + 1] or (ms[i] == ms[i + 1] and prov[i] < prov[i + 1])
        fs = fr['scores']
        assert len(set(fs.tolist())) == len(fs)
    return out


def single_boxes(views, seed=3):
    """One planted box per view and no jitter (F = 1): only the inverse transform is exercised."""
    gb = planted(5, seed)[4:5]
    V = views.shape[0]
    per_view = [[(_transform(gb, views[v])[0], np.float32(0.5 + 0.1 * v))] for v in range(V)]
    b, s, c = _pack(per_view, 4)
    return dict(boxes=b, scores=s, counts=c, views=views, F=1, ground=[gb], post_max=4)
