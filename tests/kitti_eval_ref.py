"""Host reference of the KITTI object evaluation for tests/test_kitti_eval_*.py: plain Python and numpy, written line by line
from the metric contract of DESIGN.md section 3.17 (the kitti-object-eval-python semantics).  BEV intersections come from the
C oracle's bbox_pairwise(..., iou=False) (oracle/mvx_oracle.py, read only); the corner quads from the package's shared
``bev_quads_camera``.  Deliberately slow and literal: every loop is the sequential loop of the contract."""
import numpy as np

import mvx_oracle as O
from modules.kitti_eval import bev_quads_camera

MIN_HEIGHT = (40, 25, 25)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
NEIGHBOUR = {'car': 'van', 'pedestrian': 'person_sitting'}
SETTINGS = {'car': ((0.7, 0.7, 0.7), (0.7, 0.5, 0.5)), 'pedestrian': ((0.5, 0.5, 0.5), (0.5, 0.25, 0.25)),
            'cyclist': ((0.5, 0.5, 0.5), (0.5, 0.25, 0.25))}
METRICS = ('bbox', 'bev', '3d')
DIFFS = ('easy', 'moderate', 'hard')


# ---- overlaps ------------------------------------------------------------------------------------------------------------
def image_iou(a, b, dontcare=False):
    """Axis-aligned overlap of boxes a (n,4) with b (m,4): iw*ih / (area_a + area_b - iw*ih), or / area_a for don't-cares;
    iw and ih clamped at 0, no +1; 0 where the boxes do not overlap."""
    out = np.zeros((len(a), len(b)))
    for i in range(len(a)):
        for j in range(len(b)):
            iw = max(min(a[i][2], b[j][2]) - max(a[i][0], b[j][0]), 0.0)
            ih = max(min(a[i][3], b[j][3]) - max(a[i][1], b[j][1]), 0.0)
            inter = iw * ih
            if inter <= 0.0:
                continue
            area_a = (a[i][2] - a[i][0]) * (a[i][3] - a[i][1])
            area_b = (b[j][2] - b[j][0]) * (b[j][3] - b[j][1])
            out[i, j] = inter / area_a if dontcare else inter / (area_a + area_b - inter)
    return out


def quad_circle(q):
    """bev_iou.h's bounding circle of a quad (4,2) f32, operation for operation in f32."""
    f = np.float32
    cx, cy = f(0), f(0)
    for k in range(4):
        cx = f(cx + f(f(0.25) * q[k, 0]))
        cy = f(cy + f(f(0.25) * q[k, 1]))
    r = f(0)
    for k in range(4):
        dx, dy = f(q[k, 0] - cx), f(q[k, 1] - cy)
        r = max(r, np.sqrt(f(f(dx * dx) + f(dy * dy))))
    return cx, cy, r


def circles_apart(c1, c2):
    f = np.float32
    dx, dy = f(c2[0] - c1[0]), f(c2[1] - c1[1])
    dist = np.sqrt(f(f(dx * dx) + f(dy * dy)))
    return bool(dist > f(f(f(1.01) * f(c1[2] + c2[2])) + f(1e-3)))


def frame_overlaps(dt, gt):
    """(2D, BEV, 3D) IoU matrices (n_dt, n_gt) of one frame (GT: every label row, DontCare included), and the mask of the
    pairs whose bounding circles are apart (BEV intersection 0 without clipping)."""
    nd, ng = len(dt['name']), len(gt['name'])
    iou2 = image_iou(dt['bbox'], gt['bbox'])
    dq = bev_quads_camera(dt['location'], dt['hwl'], dt['rotation_y'])
    gq = bev_quads_camera(gt['location'], gt['hwl'], gt['rotation_y'])
    inter = O.bbox_pairwise(dq, gq, False) if nd and ng else np.zeros((nd, ng), np.float32)
    apart = np.zeros((nd, ng), bool)
    dcirc = [quad_circle(q) for q in dq]
    gcirc = [quad_circle(q) for q in gq]
    bev = np.zeros((nd, ng))
    iou3 = np.zeros((nd, ng))
    for i in range(nd):
        h_d, w_d, l_d = dt['hwl'][i]
        y_d = dt['location'][i][1]
        for j in range(ng):
            h_g, w_g, l_g = gt['hwl'][j]
            y_g = gt['location'][j][1]
            apart[i, j] = circles_apart(dcirc[i], gcirc[j])
            I = 0.0 if apart[i, j] else float(inter[i, j])
            bev[i, j] = I / (l_d * w_d + l_g * w_g - I)
            ih = min(y_d, y_g) - max(y_d - h_d, y_g - h_g)
            if ih > 0:
                inc = I * ih
                iou3[i, j] = inc / (l_d * h_d * w_d + l_g * h_g * w_g - inc)
    return (iou2, bev, iou3), apart


# ---- cleaning ------------------------------------------------------------------------------------------------------------
def clean_data(gt, dt, cls, diff):
    """(ignored_gt, ignored_det, dontcare boxes, num_valid_gt) of one frame for a class and difficulty."""
    cls = cls.lower()
    ignored_gt, ignored_dt, dc = [], [], []
    n_valid = 0
    for i in range(len(gt['name'])):
        name = gt['name'][i].lower()
        height = gt['bbox'][i][3] - gt['bbox'][i][1]
        if name == cls:
            valid_class = 1
        elif name == NEIGHBOUR.get(cls):
            valid_class = 0
        else:
            valid_class = -1
        ignore = (gt['occluded'][i] > MAX_OCCLUSION[diff] or gt['truncated'][i] > MAX_TRUNCATION[diff]
                  or height <= MIN_HEIGHT[diff])
        if valid_class == 1 and not ignore:
            ignored_gt.append(0)
            n_valid += 1
        elif valid_class == 0 or (valid_class == 1 and ignore):
            ignored_gt.append(1)
        else:
            ignored_gt.append(-1)
        if name == 'dontcare':
            dc.append(gt['bbox'][i])
    for i in range(len(dt['name'])):
        height = dt['bbox'][i][3] - dt['bbox'][i][1]
        if height < MIN_HEIGHT[diff]:
            ignored_dt.append(1)
        elif dt['name'][i].lower() == cls:
            ignored_dt.append(0)
        else:
            ignored_dt.append(-1)
    return ignored_gt, ignored_dt, np.array(dc).reshape(-1, 4), n_valid


# ---- statistics ----------------------------------------------------------------------------------------------------------
def compute_statistic(overlaps, gt, dt, ignored_gt, ignored_det, dc_overlaps, metric, min_overlap, thresh=0.0,
                      compute_fp=False):
    """One frame: (tp, fp, fn, similarity, TP scores).  ``overlaps`` (n_dt, n_gt), ``dc_overlaps`` (n_dt, n_dc)."""
    det_size, gt_size = len(dt['name']), len(gt['name'])
    scores, dt_alpha, gt_alpha = dt['score'], dt['alpha'], gt['alpha']
    assigned = [False] * det_size
    ignored_threshold = [False] * det_size
    if compute_fp:
        for i in range(det_size):
            if scores[i] < thresh:
                ignored_threshold[i] = True
    tp = fp = fn = 0
    similarity = 0.0
    tp_scores, deltas = [], []
    for i in range(gt_size):
        if ignored_gt[i] == -1:
            continue
        det_idx = -1
        best = -1e7
        max_ov = 0.0
        found = False
        assigned_ignored = False
        for j in range(det_size):
            if ignored_det[j] == -1 or assigned[j] or ignored_threshold[j]:
                continue
            ov = overlaps[j, i]
            s = scores[j]
            if not compute_fp and ov > min_overlap and s > best:
                det_idx, best, found = j, s, True
            elif compute_fp and ov > min_overlap and (ov > max_ov or assigned_ignored) and ignored_det[j] == 0:
                det_idx, max_ov, found, assigned_ignored = j, ov, True, False
            elif compute_fp and ov > min_overlap and not found and ignored_det[j] == 1:
                det_idx, found, assigned_ignored = j, True, True
        if not found and ignored_gt[i] == 0:
            fn += 1
        elif found and (ignored_gt[i] == 1 or ignored_det[det_idx] == 1):
            assigned[det_idx] = True
        elif found:
            tp += 1
            tp_scores.append(scores[det_idx])
            deltas.append(gt_alpha[i] - dt_alpha[det_idx])
            assigned[det_idx] = True
    if compute_fp:
        for i in range(det_size):
            if not (assigned[i] or ignored_det[i] in (-1, 1) or ignored_threshold[i]):
                fp += 1
        nstuff = 0
        if metric == 0:
            for k in range(dc_overlaps.shape[1]):
                for j in range(det_size):
                    if assigned[j] or ignored_det[j] in (-1, 1) or ignored_threshold[j]:
                        continue
                    if dc_overlaps[j, k] > min_overlap:
                        assigned[j] = True
                        nstuff += 1
        fp -= nstuff
        if metric == 0:
            for d in deltas:
                similarity += (1.0 + np.cos(d)) / 2.0
            if tp + fp == 0:
                similarity = -1.0
    return tp, fp, fn, similarity, tp_scores


def get_thresholds(scores, num_gt, num_sample_pts=41):
    scores = sorted(scores, reverse=True)
    current_recall = 0.0
    thresholds = []
    for i, score in enumerate(scores):
        l_recall = (i + 1) / num_gt
        if i < len(scores) - 1:
            r_recall = (i + 2) / num_gt
        else:
            r_recall = l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < len(scores) - 1:
            continue
        thresholds.append(score)
        current_recall += 1 / (num_sample_pts - 1.0)
    return thresholds


def ap_r11(prec):
    s = 0.0
    for i in range(0, 41, 4):
        s += prec[i]
    return s / 11 * 100


def ap_r40(prec):
    s = 0.0
    for i in range(1, 41):
        s += prec[i]
    return s / 40 * 100


def _div(a, b):
    return a / b if b != 0 else 0.0


def evaluate(gt_annos, dt_annos, classes=('Car',)):
    """Same structure as modules.kitti_eval.evaluate: {'ap': ..., 'curves': {...}}, plus 'overlaps' (per frame (2D, BEV, 3D)
    matrices over every label row), 'apart' and 'dc_overlaps'."""
    F = len(gt_annos)
    frames = []
    for f in range(F):
        gt, dt = gt_annos[f], dt_annos[f]
        ovs, apart = frame_overlaps(dt, gt)
        frames.append((ovs, apart))
    keys, curves = [], dict(thresholds=[], n_thresholds=[], tp=[], fp=[], fn=[], similarity=[], n_gt=[])
    ap = {}
    for cls in classes:
        table = SETTINGS[cls.lower()]
        ap[cls] = [dict(min_overlaps=table[k]) for k in range(2)]
        for k in range(2):
            for m in range(3):
                for d in range(3):
                    min_overlap = table[k][m]
                    cleaned = [clean_data(gt_annos[f], dt_annos[f], cls, d) for f in range(F)]
                    dc_ovs = [image_iou(dt_annos[f]['bbox'], cleaned[f][2], dontcare=True) for f in range(F)]
                    all_scores, n_gt = [], 0
                    for f in range(F):
                        ig, idt, _, nv = cleaned[f]
                        n_gt += nv
                        all_scores += compute_statistic(frames[f][0][m], gt_annos[f], dt_annos[f], ig, idt, dc_ovs[f], m,
                                                        min_overlap)[4]
                    thresholds = get_thresholds(all_scores, n_gt)
                    pr = np.zeros((41, 4))
                    for t, thresh in enumerate(thresholds):
                        for f in range(F):
                            ig, idt, _, _ = cleaned[f]
                            tp, fp, fn, sim, _ = compute_statistic(frames[f][0][m], gt_annos[f], dt_annos[f], ig, idt, dc_ovs[f],
                                                                   m, min_overlap, thresh, True)
                            pr[t] += (tp, fp, fn, sim)
                    prec, aos = np.zeros(41), np.zeros(41)
                    for i in range(len(thresholds)):
                        prec[i] = _div(pr[i, 0], pr[i, 0] + pr[i, 1])
                        aos[i] = _div(pr[i, 3], pr[i, 0] + pr[i, 1])
                    for i in range(41):
                        prec[i] = np.max(prec[i:])
                        aos[i] = np.max(aos[i:])
                    keys.append((cls, k, METRICS[m], DIFFS[d]))
                    curves['thresholds'].append(np.array(thresholds + [0.0] * (41 - len(thresholds))))
                    curves['n_thresholds'].append(len(thresholds))
                    for c, name in enumerate(('tp', 'fp', 'fn', 'similarity')):
                        curves[name].append(pr[:, c])
                    curves['n_gt'].append(n_gt)
                    e = ap[cls][k].setdefault(METRICS[m], {'R11': [0.0] * 3, 'R40': [0.0] * 3})
                    e['R11'][d], e['R40'][d] = ap_r11(prec), ap_r40(prec)
                    if m == 0:
                        e = ap[cls][k].setdefault('aos', {'R11': [0.0] * 3, 'R40': [0.0] * 3})
                        e['R11'][d], e['R40'][d] = ap_r11(aos), ap_r40(aos)
    out = {name: np.array(v) for name, v in curves.items()}
    for name in ('tp', 'fp', 'fn'):
        out[name] = out[name].astype(np.int64)
    out['keys'] = keys
    dc_all = [image_iou(dt_annos[f]['bbox'], clean_data(gt_annos[f], dt_annos[f], classes[0], 0)[2], dontcare=True)
              for f in range(F)]
    return dict(ap=ap, curves=out, overlaps=[fr[0] for fr in frames], apart=[fr[1] for fr in frames], dc_overlaps=dc_all)
