"""Host reference of the detection output for tests/test_detect_gpu.py and tests/test_detect_direct_gpu.py: candidate order and
selection in numpy, decoding in float64, greedy NMS on the C oracle's rotated IoU (oracle/mvx_oracle.py, read only), over the
whole IoU table (``greedy_nms``) or over the pairs that can touch (``greedy_nms_near``, for thousands of boxes)."""
import numpy as np
import torch

import mvx_oracle as O


def candidates(logits, score_thr, pre_max):
    """logits f32 (N,) of one frame -> (anchor indices of the candidates in order, number above the threshold): selection
    by torch.sigmoid(logit) >= score_thr, order logit descending then index ascending, the first pre_max."""
    lg = np.asarray(logits, np.float32)
    sel = (torch.sigmoid(torch.from_numpy(lg)) >= score_thr).numpy()
    idx = np.nonzero(sel)[0]
    order = np.lexsort((idx, -lg[idx].astype(np.float64)))
    return idx[order][:pre_max], int(sel.sum())


def encode(gt, anchor):
    """VoxelLoss's regression targets (voxelnet/Loss.py:35-40, csrc/loss.hip) of a box for an anchor, float64."""
    g, a = np.asarray(gt, np.float64), np.asarray(anchor, np.float64)
    d = np.sqrt(a[3] ** 2 + a[4] ** 2)
    return np.array([(g[0] - a[0]) / d, (g[1] - a[1]) / d, (g[2] - a[2]) / a[5], np.log(g[3] / a[3]), np.log(g[4] / a[4]),
                     np.log(g[5] / a[5]), g[6] - a[6]])


def decode(reg, anchors, mode):
    """(n,7) regressions and anchors -> boxes in float64; 'loss' = inverse of ``encode``, 'reference' = Calc.decodeRegression
    (diagonal of anchor columns 0:2)."""
    r, a = np.asarray(reg, np.float64), np.asarray(anchors, np.float64)
    d = np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2) if mode == 'reference' else np.sqrt(a[:, 3] ** 2 + a[:, 4] ** 2)
    out = np.empty_like(r)
    out[:, 0] = r[:, 0] * d + a[:, 0]
    out[:, 1] = r[:, 1] * d + a[:, 1]
    out[:, 2] = r[:, 2] * a[:, 5] + a[:, 2]
    out[:, 3:6] = np.exp(r[:, 3:6]) * a[:, 3:6]
    out[:, 6] = r[:, 6] + a[:, 6]
    return out


def decode_scale(reg, anchors, mode):
    """Magnitude of the f32 operands behind every decoded component (the sum of the two terms of x, y, z; the value
    itself for the others): an f32 decode is within a few ulp of this, also where the two terms cancel."""
    r, a = np.abs(np.asarray(reg, np.float64)), np.abs(np.asarray(anchors, np.float64))
    out = np.abs(decode(reg, anchors, mode))
    d = np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2) if mode == 'reference' else np.sqrt(a[:, 3] ** 2 + a[:, 4] ** 2)
    out[:, 0] = r[:, 0] * d + a[:, 0]
    out[:, 1] = r[:, 1] * d + a[:, 1]
    out[:, 2] = r[:, 2] * a[:, 5] + a[:, 2]
    out[:, 6] = r[:, 6] + a[:, 6]
    return np.maximum(out, 1.0)


def corners(boxes):
    """(n,7) -> (n,4,2) with the oracle's bbox3d2bev (f32 torch on the host)."""
    return O.bbox3d2bev(torch.as_tensor(np.asarray(boxes, np.float32))).numpy()


def greedy_nms(quads, iou_thr, post_max):
    """Greedy NMS over quads (K,4,2) in the given order: j is suppressed by a kept i < j when IoU(i, j) > iou_thr, the IoU
    of box i against box j from the C oracle (cpp.bboxOverlap's arithmetic).  Returns the kept positions."""
    K = quads.shape[0]
    if K == 0:
        return []
    iou = O.bbox_pairwise(quads, quads, True)
    removed = np.zeros(K, bool)
    keep = []
    for i in range(K):
        if removed[i]:
            continue
        keep.append(i)
        if len(keep) == post_max:
            break
        removed[i + 1:] |= iou[i, i + 1:] > iou_thr
    return keep


def near_pairs(quads):
    """The IoU table of ``greedy_nms`` without its empty part: per box i (the partners j, IoU(i, j) from the C oracle) for the
    pairs whose float64 bounding circles (centre = mean corner, radius = farthest corner) come within 10 % + 1 cm of touching,
    dist <= 1.1 (r_i + r_j) + 0.01.  Every other pair is disjoint, IoU 0 -- below any iou_thr >= 1e-3, where the oracle itself
    gives rounding noise of ~1e-6.  The centres are bucketed into square cells as wide as the largest such distance, and the
    oracle is called per cell against its 3 x 3 neighbourhood."""
    q = np.ascontiguousarray(quads, np.float32)
    n = q.shape[0]
    q64 = q.astype(np.float64)
    c = q64.mean(1)
    r = np.sqrt(((q64 - c[:, None]) ** 2).sum(2)).max(1)
    cell = 2.2 * r.max() + 0.01
    ij = np.floor((c - c.min(0)) / cell).astype(np.int64)
    cells = {}
    for k, key in enumerate(map(tuple, ij)):
        cells.setdefault(key, []).append(k)
    cols, ious = [None] * n, [None] * n
    for (cx, cy), rows in cells.items():
        rows = np.array(rows)
        part = np.array([k for dx in (-1, 0, 1) for dy in (-1, 0, 1) for k in cells.get((cx + dx, cy + dy), ())])
        iou = O.bbox_pairwise(q[rows], q[part], True)
        dist = np.sqrt(((c[rows][:, None] - c[part][None]) ** 2).sum(2))
        near = (dist <= 1.1 * (r[rows][:, None] + r[part][None]) + 0.01) & (rows[:, None] != part[None])
        for a, i in enumerate(rows):
            cols[i], ious[i] = part[near[a]], iou[a, near[a]]
    return cols, ious


def greedy_nms_near(quads, iou_thr, post_max, pairs=None):
    """``greedy_nms`` from the IoUs of ``near_pairs`` alone (iou_thr >= 1e-3): the same kept positions without the K x K table."""
    assert iou_thr >= 1e-3
    K = quads.shape[0]
    if K == 0:
        return []
    cols, ious = near_pairs(quads) if pairs is None else pairs
    removed = np.zeros(K, bool)
    keep = []
    for i in range(K):
        if removed[i]:
            continue
        keep.append(i)
        if len(keep) == post_max:
            break
        hit = cols[i][(ious[i] > iou_thr) & (cols[i] > i)]
        removed[hit] = True
    return keep
