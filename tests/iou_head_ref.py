"""Float64 restatement of the IoU-aware confidence head (include/mvx_hip.h mvx_focal_loss_iou_frames / mvx_detect_frames_iou,
DESIGN.md 3.35), built on focal_ref.py, direction_ref.py and detect_ref.py by import.

    targets(case)            -> per-entry IoU targets q f64 (F,cap) (-1 = skipped / unused) and the masks the tests compare by
    iou_head_ref(case, ...)  -> (losses f64 (F,4), d_heads f64 (F*l*w, 8A), d_dir, d_iou f64 (F*l*w, A), q)      closed form
    iou_head_autograd(case)  -> the IoU loss and its gradient from torch.autograd on a float64 restatement
    rectified_log / candidates                                                           the decode's score, order, selection
    q_f32(case)              -> the same targets in the project's accepted f32 arithmetic (the C oracle's clipping)

``case`` is a direction_ref case plus ``iou`` f32 (F*l*w, A), the IoU logits.  The classification, regression and direction
terms are direction_ref's own (called, not restated).
"""
import math

import numpy as np
import torch
import torch.nn.functional as Fn

import detect_ref as D
import direction_ref as DR

ZERO_MARGIN = 1e-3          # an entry counts as "exactly 0" only when its reason holds by this margin (metres)


# ---- the exact convex clip ------------------------------------------------------------------------------------------------
def quad64(box):
    """BEV corners (4,2) f64 of a box xyzlwhr, Calc.bbox3d2bev's formula: unit corners scaled by (l, w), times
    [[cos, -sin], [sin, cos]] from the right, shifted by (x, y)."""
    b = np.asarray(box, np.float64)
    unit = np.array([[0.5, 0.5], [-0.5, 0.5], [-0.5, -0.5], [0.5, -0.5]]) * b[3:5]
    c, s = math.cos(b[6]), math.sin(b[6])
    return unit @ np.array([[c, -s], [s, c]]) + b[0:2]


def _area(poly):
    x, y = poly[:, 0], poly[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - y * np.roll(x, -1)))


def clip_area(qa, qb):
    """Area of the intersection of two convex quads (4,2) f64: Sutherland-Hodgman, qa clipped by the edges of qb."""
    qa, qb = np.asarray(qa, np.float64), np.asarray(qb, np.float64)
    if _area(qa) < 0:
        qa = qa[::-1]
    if _area(qb) < 0:
        qb = qb[::-1]
    poly = [p for p in qa]
    for i in range(4):
        a, b = qb[i], qb[(i + 1) % 4]
        side = [(b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]) for p in poly]
        nxt = []
        for k in range(len(poly)):
            p, q, sp, sq = poly[k], poly[(k + 1) % len(poly)], side[k], side[(k + 1) % len(poly)]
            if sp >= 0:
                nxt.append(p)
            if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
                nxt.append(p + (q - p) * (sp / (sp - sq)))
        poly = nxt
        if len(poly) < 3:
            return 0.0
    return abs(_area(np.array(poly)))


def circle_gap(qa, qb):
    """dist - (1.01 (r1 + r2) + 1e-3) of the bounding circles (bev_iou.h circles_apart): > 0 = rejected."""
    ca, cb = qa.mean(0), qb.mean(0)
    ra, rb = np.sqrt(((qa - ca) ** 2).sum(1)).max(), np.sqrt(((qb - cb) ** 2).sum(1)).max()
    return float(np.sqrt(((ca - cb) ** 2).sum()) - (1.01 * (ra + rb) + 1e-3))


def iou3d(b, g):
    """(q, info) of a decoded box b and a ground truth g, xyzlwhr f64 with z the bottom face: the 3D IoU clamped to [0, 1], 0
    when the bounding circles cannot touch or the vertical overlap is <= 0.  info = (circle gap, ih, BEV intersection)."""
    qa, qb = quad64(b), quad64(g)
    gap = circle_gap(qa, qb)
    ih = min(b[2] + b[5], g[2] + g[5]) - max(b[2], g[2])
    inter = 0.0 if gap > 0 else clip_area(qa, qb)
    if gap > 0 or ih <= 0:
        return 0.0, (gap, ih, inter)
    vol = inter * ih
    v = vol / (b[3] * b[4] * b[5] + g[3] * g[4] * g[5] - vol)
    return (min(max(v, 0.0), 1.0) if math.isfinite(v) else 0.0), (gap, ih, inter)


def _entry_rows(case, f):
    """The pos_idx slots of frame f: (slot k, x, y, z, row of gts) for the entries the regression term takes."""
    l, w, A = case['l'], case['w'], case['A']
    n_pos = int(case['counts'][f, 0])
    n_gt = int(case['gt_off'][f + 1]) - int(case['gt_off'][f])
    out = []
    for k in range(n_pos):
        x, y, z = (int(case['pos'][f, j, k]) for j in range(3))
        g = int(case['gi'][f, k])
        if 0 <= x < l and 0 <= y < w and 0 <= z < A and 0 <= g < n_gt:
            out.append((k, x, y, z, int(case['gt_off'][f]) + g))
    return out


def targets(case):
    """q f64 (F,cap), -1 for skipped entries and unused slots, and per listed entry a record
    dict(f, k, x, y, z, q, gap, ih, inter, finite): ``finite`` = every component of the f32 decode is finite."""
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    cap = case['gi'].shape[1]
    heads = np.asarray(case['heads'], np.float32).reshape(F, l, w, -1)
    an = np.asarray(case['anchors'], np.float32).reshape(l, w, A, 7)
    gts = np.asarray(case['gts'], np.float64)
    q = np.full((F, cap), -1.0)
    recs = []
    for f in range(F):
        for k, x, y, z, row in _entry_rows(case, f):
            r = heads[f, x, y, A + 7 * z:A + 7 * z + 7]
            with np.errstate(over='ignore'):
                b32 = np.concatenate([r[0:2] * np.sqrt(an[x, y, z, 3] ** 2 + an[x, y, z, 4] ** 2), r[2:3] * an[x, y, z, 5],
                                      np.exp(r[3:6]) * an[x, y, z, 3:6], r[6:7]])
            finite = bool(np.isfinite(b32).all())
            if finite:
                b = D.decode(r[None].astype(np.float64), an[x, y, z][None].astype(np.float64), 'loss')[0]
                val, (gap, ih, inter) = iou3d(b, gts[row, :7])
            else:
                val, gap, ih, inter = 0.0, float('nan'), float('nan'), float('nan')
            q[f, k] = val
            recs.append(dict(f=f, k=k, x=x, y=y, z=z, row=row, q=val, gap=gap, ih=ih, inter=inter, finite=finite))
    return q, recs


def must_be_zero(rec):
    """The entry's q is 0 on the device bit for bit: an overflowing decode, circles apart or no vertical overlap, by a margin."""
    return (not rec['finite']) or rec['gap'] > ZERO_MARGIN or rec['ih'] < -ZERO_MARGIN


def q_f32(case, recs):
    """q of every listed entry in the project's accepted f32 arithmetic: the f32 decode, O.bbox3d2bev quads, the C oracle's
    intersection (cpp.bboxIntersection's arithmetic), the vertical term and the quotient in f32.  NaN where must_be_zero."""
    import mvx_oracle as O
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    heads = np.asarray(case['heads'], np.float32).reshape(F, l, w, -1)
    an = np.asarray(case['anchors'], np.float32).reshape(l, w, A, 7)
    gts = np.asarray(case['gts'], np.float32)
    out = np.full(len(recs), np.nan)
    for i, rec in enumerate(recs):
        if must_be_zero(rec):
            continue
        f, x, y, z = rec['f'], rec['x'], rec['y'], rec['z']
        r, a = heads[f, x, y, A + 7 * z:A + 7 * z + 7], an[x, y, z]
        d = np.sqrt(a[3] * a[3] + a[4] * a[4], dtype=np.float32)
        b = np.array([r[0] * d + a[0], r[1] * d + a[1], r[2] * a[5] + a[2], np.exp(r[3]) * a[3], np.exp(r[4]) * a[4],
                      np.exp(r[5]) * a[5], r[6] + a[6]], np.float32)
        g = gts[rec['row'], :7]
        ih = np.float32(min(b[2] + b[5], g[2] + g[5]) - max(b[2], g[2]))
        if rec['gap'] > 0 or ih <= 0:
            out[i] = 0.0
            continue
        quads = O.bbox3d2bev(torch.from_numpy(np.stack([b, g]))).numpy()
        inter = np.float32(O.bbox_pairwise(quads[0:1], quads[1:2], False)[0, 0])
        vol = np.float32(inter * ih)
        v = np.float32(vol / np.float32(np.float32(b[3] * b[4] * b[5]) + np.float32(g[3] * g[4] * g[5]) - vol))
        out[i] = float(min(max(v, np.float32(0)), np.float32(1))) if np.isfinite(v) else 0.0
    return out


# ---- the loss ---------------------------------------------------------------------------------------------------------------
def iou_head_ref(case, alpha=0.25, gamma=2.0, cls_weight=1.0, reg_weight=2.0, dir_weight=0.2, dir_offset=math.pi / 4,
                 iou_weight=1.0, q=None):
    """losses (F,4) = (cls, reg, dir, iou), d_heads, d_dir (direction_ref's own), d_iou in closed form, q (F,cap)."""
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    base = DR.direction_ref(case, alpha, gamma, cls_weight, reg_weight, True, dir_weight, dir_offset)
    if q is None:
        q = targets(case)[0]
    losses = torch.zeros((F, 4), dtype=torch.float64)
    losses[:, :3] = base[0]
    logits = np.asarray(case['iou'], np.float64).reshape(F, l, w, A)
    d_iou = np.zeros((F, l, w, A))
    for f in range(F):
        n_pos = int(case['counts'][f, 0])
        scale = iou_weight / max(1, n_pos)
        total = 0.0
        for k, x, y, z, _ in _entry_rows(case, f):
            u, t = logits[f, x, y, z], q[f, k]
            total += max(u, 0.0) + math.log1p(math.exp(-abs(u))) - t * u                  # softplus(u) - q u
            e = math.exp(-abs(u))
            d_iou[f, x, y, z] += scale * ((1.0 / (1.0 + e) if u >= 0 else e / (1.0 + e)) - t)
        losses[f, 3] = scale * total
    return losses, base[1], base[2], torch.from_numpy(d_iou.reshape(F * l * w, A)), q


def iou_head_autograd(case, iou_weight=1.0, q=None):
    """The IoU term written forward only in float64 torch: BCE with logits on the soft target q (a constant)."""
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    if q is None:
        q = targets(case)[0]
    logits = torch.from_numpy(np.asarray(case['iou'], np.float64)).reshape(F, l, w, A).requires_grad_(True)
    losses = []
    for f in range(F):
        ent = _entry_rows(case, f)
        n_pos = int(case['counts'][f, 0])
        if not ent:
            losses.append(logits.sum() * 0.0)
            continue
        ks, xs, ys, zs = (torch.tensor([e[j] for e in ent]) for j in range(4))
        t = torch.from_numpy(q[f])[ks]
        losses.append(iou_weight / max(1, n_pos) * Fn.binary_cross_entropy_with_logits(logits[f][xs, ys, zs], t, reduction='sum'))
    losses = torch.stack(losses)
    losses.sum().backward()
    return losses.detach(), logits.grad.reshape(F * l * w, A)


# ---- the decode -------------------------------------------------------------------------------------------------------------
def _softplus_neg(x):
    x = np.asarray(x, np.float64)
    return np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def rectified_log(cls, iou, a):
    """s = -((1 - a) softplus(-c) + a softplus(-u)) in float64: the log of cls^(1-a) iou^a."""
    return -((1.0 - a) * _softplus_neg(cls) + a * _softplus_neg(iou))


def candidates(cls, iou, a, score_thr, pre_max):
    """Logits f32 (N,) of one frame -> (anchor indices in order, their scores exp(s), number admitted): admitted when
    exp(s) >= score_thr (a NaN fails), order s descending then index ascending, the first pre_max."""
    s = rectified_log(np.asarray(cls, np.float32), np.asarray(iou, np.float32), a)
    with np.errstate(invalid='ignore'):
        sel = np.exp(s) >= score_thr
    idx = np.nonzero(sel)[0]
    order = np.lexsort((idx, -s[idx]))
    keep = idx[order][:pre_max]
    return keep, np.exp(s[keep]), int(sel.sum())
