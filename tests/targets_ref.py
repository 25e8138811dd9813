"""Independent float64 references of the label path (csrc/bev_iou.h, csrc/anchors.hip, csrc/loss.hip) for
tests/test_targets_direct_host.py and tests/test_targets_direct_gpu.py.

poly_iou64: the geometric truth of the BEV IoU -- Sutherland-Hodgman clipping of one convex quad by the other in float64 on
the f32 corner values, shoelace areas.  No origin fan, no tolerance.
circles_apart32: numpy f32 restatement of the kernels' bounding-circle shortcut (bev_iou.h).
voxel_loss64: the formulas of the header comment of loss.hip in float64 with closed-form gradients.  The order and the f32
IoU arithmetic of the anchor walk have their bit-exact reference in oracle/anchors_c.c and are not restated here."""
import numpy as np


def _area64(p):
    x, y = p[:, 0], p[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - y * np.roll(x, -1)))


def _clip64(subject, clip):
    """Convex ``subject`` (k,2) cut by every edge of the counter-clockwise convex ``clip``; points ON an edge are inside."""
    out = [tuple(p) for p in subject]
    n = clip.shape[0]
    for e in range(n):
        if not out:
            break
        ax, ay = clip[e]
        bx, by = clip[(e + 1) % n]
        src, out = out, []
        side = [(bx - ax) * (py - ay) - (by - ay) * (px - ax) for px, py in src]
        for i, (p, sp) in enumerate(zip(src, side)):
            q, sq = src[(i + 1) % len(src)], side[(i + 1) % len(src)]
            if sp >= 0:
                out.append(p)
            if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return np.array(out, np.float64).reshape(-1, 2)


def poly_iou64(qa, qb):
    """(intersection area, IoU) of two convex quads given as 8 f32 values each, either winding.  The clipping is done both
    ways and the smaller area taken: of two disjoint convex polygons one has an edge whose line separates them, and the
    clipping by that polygon then ends with no vertex at all, so disjoint quads give exactly 0."""
    a = np.asarray(qa, np.float32).astype(np.float64).reshape(4, 2)
    b = np.asarray(qb, np.float32).astype(np.float64).reshape(4, 2)
    if _area64(a) < 0:
        a = a[::-1]
    if _area64(b) < 0:
        b = b[::-1]
    ab, ba = _clip64(a, b), _clip64(b, a)
    inter = min(abs(_area64(ab)) if len(ab) > 2 else 0.0, abs(_area64(ba)) if len(ba) > 2 else 0.0)
    return inter, inter / (_area64(a) + _area64(b) - inter)


def circles_apart32(qa, qb):
    """bev_iou.h quad_circle + circles_apart in numpy f32, operation for operation.  qa, qb (..., 4, 2) f32 -> bool (...)."""
    f = np.float32

    def circle(q):
        q = np.asarray(q, f)
        cx, cy = np.zeros(q.shape[:-2], f), np.zeros(q.shape[:-2], f)
        for k in range(4):
            cx = cx + f(0.25) * q[..., k, 0]
            cy = cy + f(0.25) * q[..., k, 1]
        r = np.zeros(q.shape[:-2], f)
        for k in range(4):
            dx, dy = q[..., k, 0] - cx, q[..., k, 1] - cy
            r = np.maximum(r, np.sqrt(dx * dx + dy * dy))
        return cx, cy, r
    (ax, ay, ar), (bx, by, br) = circle(qa), circle(qb)
    dx, dy = bx - ax, by - ay
    dist = np.sqrt(dx * dx + dy * dy)
    return dist > f(1.01) * (ar + br) + f(1e-3)


def targets32(g, an):
    """Regression targets t[0..7) of ground truths g (n, >= 7) against anchors an (n, 7), formed in f32 as loss.hip does."""
    f = np.float32
    g, an = np.asarray(g, f), np.asarray(an, f)
    d = np.sqrt(an[:, 3] * an[:, 3] + an[:, 4] * an[:, 4])
    t = np.empty((g.shape[0], 7), f)
    t[:, 0] = (g[:, 0] - an[:, 0]) / d
    t[:, 1] = (g[:, 1] - an[:, 1]) / d
    t[:, 2] = (g[:, 2] - an[:, 2]) / an[:, 5]
    t[:, 3:6] = np.log(g[:, 3:6] / an[:, 3:6])
    t[:, 6] = g[:, 6] - an[:, 6]
    return t


def voxel_loss64(score, reg, pos, neg, gi, gts, anchors, a=1.5, b=1.0, eps=1e-6, f32_roundings=True):
    """VoxelLoss forward and backward.  score (L,W,A) f32, reg (L,W,7A) f32 or None, pos / neg i64 (3, n) index triples (neg =
    the NOT-negative anchors), gi (n_pos,), gts (n, >= 7), anchors (L,W,A,7).
    Returns (losses f64 (2,) = (clsLoss, regLoss), dscore f64 (L,W,A), dreg f64 (L,W,7A) or None).

    With ``f32_roundings`` the roundings loss.hip documents are reproduced and nothing else: om = 1f - s + eps and sp = s + eps
    in f32, the two denominators rounded to f32, the targets in f32.  Logs, sums and SmoothL1 are float64.  Without it every
    step is float64 (used to check the closed-form gradients against autograd)."""
    f = np.float32 if f32_roundings else np.float64
    score = np.asarray(score, np.float32)
    L, W, A = score.shape
    N = L * W * A
    pos = np.asarray(pos, np.int64).reshape(3, -1)
    neg = np.asarray(neg, np.int64).reshape(3, -1)
    n_pos, n_neg = pos.shape[1], neg.shape[1]
    e = f(np.float32(eps))
    s = score.astype(f)
    om = ((f(1.0) - s) + e).astype(np.float64)
    sp = (s + e).astype(np.float64)
    den_pos = float(f(float(n_pos) + float(e)))
    den_neg = float(f(float(N - n_neg) + float(e)))
    a, b = float(np.float32(a)), float(np.float32(b))
    neg_all = -np.log(om)
    pi, ni = tuple(pos), tuple(neg)
    pos_loss = float(np.sum(-np.log(sp[pi]))) / den_pos
    neg_loss = (float(np.sum(neg_all)) - float(np.sum(neg_all[ni]))) / den_neg
    dscore = b / den_neg / om
    np.add.at(dscore, ni, -(b / den_neg) / om[ni])                     # duplicates add up
    np.add.at(dscore, pi, -(a / den_pos) / sp[pi])
    losses = np.array([a * pos_loss + b * neg_loss, 0.0])
    if reg is None:
        return losses, dscore, None
    reg = np.asarray(reg, np.float32)
    dreg = np.zeros((L, W, A, 7), np.float64)
    if n_pos > 0:
        an = np.asarray(anchors, np.float32).reshape(L, W, A, 7)[pi]
        g = np.asarray(gts, np.float32)[np.asarray(gi, np.int64)][:, :7]
        t = targets32(g, an).astype(np.float64) if f32_roundings else _targets64(g, an)
        diff = reg.reshape(L, W, A, 7)[pi].astype(np.float64) - t
        ad = np.abs(diff)
        losses[1] = float(np.sum(np.where(ad < 1.0, 0.5 * diff * diff, ad - 0.5))) / (7.0 * n_pos)
        np.add.at(dreg, pi, np.where(ad < 1.0, diff, np.sign(diff)) / (7.0 * n_pos))
    return losses, dscore, dreg.reshape(L, W, 7 * A)


def _targets64(g, an):
    g, an = g.astype(np.float64), an.astype(np.float64)
    d = np.sqrt(an[:, 3] ** 2 + an[:, 4] ** 2)
    t = np.empty((g.shape[0], 7))
    t[:, 0] = (g[:, 0] - an[:, 0]) / d
    t[:, 1] = (g[:, 1] - an[:, 1]) / d
    t[:, 2] = (g[:, 2] - an[:, 2]) / an[:, 5]
    t[:, 3:6] = np.log(g[:, 3:6] / an[:, 3:6])
    t[:, 6] = g[:, 6] - an[:, 6]
    return t
