"""Float64 restatement of the test-time augmentation's fusion (csrc/tta.hip, modules/tta.py) for tests/test_tta_*.py: the
inverse view transform, the merged order, the pairwise IoU (the C oracle's rotated IoU on the oracle's corners, as
tests/detect_ref.py takes it), heads, ownership, votes, the weighted averages and the final order."""
import math

import numpy as np

import detect_ref as D

PI = math.pi


def wrap(r, period):
    """r into [-period/2, period/2)."""
    return r - period * np.floor((r + 0.5 * period) / period)


def is_identity(row):
    row = np.asarray(row, np.float32)
    return row[0] == 0 and row[1] == 1 and row[2] == 0


def inverse_boxes(boxes, row):
    """Boxes (n,7) of a view back in the source frame, float64: the inverse of ``Geometry.transform_boxes`` for the row
    (phi, s, flip, 0).  The inputs are taken as the f32 numbers they are."""
    b = np.asarray(boxes, np.float32).astype(np.float64).reshape(-1, 7)
    row = np.asarray(row, np.float32).astype(np.float64)
    if is_identity(row):
        return b.copy()
    phi, s, flip = row[0], row[1], row[2] != 0
    x, y, r = b[:, 0].copy(), b[:, 1].copy(), b[:, 6].copy()
    if flip:
        y, r = -y, -r
    c, sn = math.cos(phi), math.sin(phi)
    out = np.empty_like(b)
    out[:, 0] = (c * x - sn * y) / s
    out[:, 1] = (sn * x + c * y) / s
    out[:, 2] = b[:, 2] / s
    out[:, 3:6] = b[:, 3:6] / s
    out[:, 6] = wrap(r - phi, 2 * PI)
    return out


def merge(boxes, scores, counts, views):
    """One source frame: boxes (V, post_max, 7), scores (V, post_max), counts (V,), views (V, 4) -> (boxes f64 (n,7) in the
    source frame, scores f64 (n,), prov (n,) = view * post_max + rank) in merged order: score descending, then view, then rank.
    Entries with a non-finite box or score are left out; the flag says whether there was one."""
    V, post_max = scores.shape
    bs, ss, pv, bad = [], [], [], False
    for v in range(V):
        n = int(min(max(counts[v], 0), post_max))
        with np.errstate(all='ignore'):         # non-finite entries are met on purpose
            back = inverse_boxes(boxes[v, :n], views[v]).astype(np.float32).astype(np.float64)      # the kernel rounds once here
        for k in range(n):
            if np.isfinite(back[k]).all() and np.isfinite(scores[v, k]):
                bs.append(back[k]); ss.append(float(np.float32(scores[v, k]))); pv.append(v * post_max + k)
            else:
                bad = True
    if not bs:
        return np.zeros((0, 7)), np.zeros((0,)), np.zeros((0,), np.int64), bad
    bs, ss, pv = np.array(bs), np.array(ss), np.array(pv)
    order = np.lexsort((pv, -ss))
    return bs[order], ss[order], pv[order], bad


def iou_matrix(boxes):
    """Pairwise BEV IoU (n, n) of boxes (n,7), row i against column j."""
    if boxes.shape[0] == 0:
        return np.zeros((0, 0))
    q = D.corners(boxes)
    return np.asarray(D.O.bbox_pairwise(q, q, True), np.float64)


def clusters(iou, prov, post_max, iou_thr, fuse_iou):
    """(heads, owner (n,), voters per head in merged order) of the greedy scan."""
    n = iou.shape[0]
    owner = np.full(n, -1)
    heads = []
    for i in range(n):
        for h in heads:
            if iou[h, i] > iou_thr:
                owner[i] = h
                break
        else:
            heads.append(i)
    voters = {}
    for h in heads:
        seen = {prov[h] // post_max}
        vs = [h]
        for j in range(h + 1, n):
            if owner[j] == h and iou[h, j] > fuse_iou and prov[j] // post_max not in seen:
                seen.add(prov[j] // post_max)
                vs.append(j)
        voters[h] = vs
    return heads, owner, voters


def fuse_frame(boxes, scores, counts, views, iou_thr, fuse_iou, min_views, out_max, full_turn):
    """One source frame -> dict(boxes f64 (m,7), scores f64 (m,), n_views, src, heads (merged positions), bad, iou, merged)."""
    V, post_max = scores.shape
    mb, ms, prov, bad = merge(boxes, scores, counts, views)
    iou = iou_matrix(mb)
    heads, owner, voters = clusters(iou, prov, post_max, iou_thr, fuse_iou)
    period = 2 * PI if full_turn else PI
    rows = []
    for h in heads:
        vs = voters[h]
        w = ms[vs]
        if len(vs) == 1 or not w.sum() > 0:
            box = mb[h].copy()
        else:
            box = np.empty(7)
            box[:6] = (w[:, None] * mb[vs, :6]).sum(0) / w.sum()
            d = wrap(mb[vs, 6] - mb[h, 6], period)
            box[6] = wrap(mb[h, 6] + (w * d).sum() / w.sum(), 2 * PI)
        score = float(np.float32(w.sum() / V))
        if len(vs) >= min_views:
            rows.append((score, h, box, len(vs)))
    rows.sort(key=lambda t: (-t[0], t[1]))
    rows = rows[:out_max]
    return dict(boxes=np.array([r[2] for r in rows]).reshape(-1, 7), scores=np.array([r[0] for r in rows]),
                n_views=np.array([r[3] for r in rows], np.int64), src=np.array([prov[r[1]] for r in rows], np.int64),
                heads=[r[1] for r in rows], bad=bad, iou=iou, merged=(mb, ms, prov), all_heads=heads, voters=voters)


def fuse(boxes, scores, counts, views, F, iou_thr, fuse_iou=0.5, min_views=1, out_max=None, full_turn=False):
    """boxes (F*V, post_max, 7), scores (F*V, post_max), counts (F*V,), views (V, 4) -> the list of ``fuse_frame`` per source frame."""
    views = np.asarray(views, np.float32)
    V, post_max = views.shape[0], scores.shape[1]
    out_max = post_max if out_max is None else out_max
    return [fuse_frame(boxes[f * V:(f + 1) * V], scores[f * V:(f + 1) * V], counts[f * V:(f + 1) * V], views, iou_thr, fuse_iou,
                       min_views, out_max, full_turn) for f in range(F)]


def yaw_distance(a, b):
    """|a - b| modulo 2 pi."""
    return np.abs(wrap(np.asarray(a, np.float64) - np.asarray(b, np.float64), 2 * PI))
