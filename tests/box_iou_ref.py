"""Restatements of the rotated 3D IoU regression loss (include/mvx_hip.h mvx_box_iou_loss_frames, csrc/box_iou_loss.hip,
DESIGN.md 3.36).  The reference project has no such loss: these ARE the yardstick.

    q_ref(case, weight)          (a) q f64 (F,cap) (-1 = skipped / unused), out f64 (F,2) = (term, mean q): the 'loss' decode in
                                     float64 and iou_head_ref.iou3d (world-coordinate Sutherland-Hodgman), nothing else
    loss_autograd(case, weight)  (b) the same written in float64 torch, so that autograd gives d(sum of the terms)/d(heads):
                                     a Sutherland-Hodgman loop over torch scalars
    central_differences(...)         d/d(heads) of (a) by central differences, entry by entry
    kernel_restated(case, weight, T) the KERNEL's own algorithm (centre difference first, clip in the predicted box's frame,
                                     tagged edges, boundary integrals, chain rule) in numpy scalars of type T: np.float32 sets
                                     the error bars of the GPU tests, np.float64 is held against (a) and (b) on the host

``case``: dict(F, l, w, A, heads f32 (F*l*w, ld), anchors f32 (l,w,A,7), pos i64 (F,3,cap), gi i64 (F,cap), counts i32 (F,2),
gts f32 (n,7), gt_off i32 (F+1,)) -- the keys of the focal / IoU-head cases.
"""
import math

import numpy as np
import torch

import iou_head_ref as IR


def entries(case, f):
    """(slot k, x, y, z, row of gts) of the pos_idx entries of frame f that are taken (iou_head_ref's rule)."""
    return IR._entry_rows(case, f)


def reg_row(case, f, x, y, z):
    """The anchor's seven regression values (f32) and its first column in the head rows."""
    l, w, A = case['l'], case['w'], case['A']
    col = A + 7 * z
    return case['heads'][(f * l + x) * w + y, col:col + 7], col


def decode64(r, an):
    """The 'loss' decode in float64 from f32 operands."""
    r, an = np.asarray(r, np.float64), np.asarray(an, np.float64)
    d = math.sqrt(an[3] ** 2 + an[4] ** 2)
    with np.errstate(over='ignore'):
        return np.array([r[0] * d + an[0], r[1] * d + an[1], r[2] * an[5] + an[2], math.exp(min(r[3], 1e3)) * an[3],
                         math.exp(min(r[4], 1e3)) * an[4], math.exp(min(r[5], 1e3)) * an[5], r[6] + an[6]])


def finite_f32(r, an):
    """Is every component of the f32 decode finite (the kernel's test)?"""
    r, an = np.asarray(r, np.float32), np.asarray(an, np.float32)
    with np.errstate(over='ignore'):
        b = np.concatenate([r[0:2] * np.sqrt(an[3] * an[3] + an[4] * an[4]) + an[0:2], r[2:3] * an[5] + an[2],
                            np.exp(r[3:6]) * an[3:6], r[6:7] + an[6]])
    return bool(np.isfinite(b).all())


def q_of_row(r, an, g):
    """q of one entry in float64: 0 when the f32 decode or the box is not finite."""
    if not finite_f32(r, an) or not np.isfinite(np.asarray(g, np.float64)).all():
        return 0.0
    return IR.iou3d(decode64(r, an), np.asarray(g, np.float64)[:7])[0]


# ---- (a) ----------------------------------------------------------------------------------------------------------------------
def q_ref(case, weight=1.0):
    F = case['F']
    cap = case['gi'].shape[1]
    q = np.full((F, cap), -1.0)
    out = np.zeros((F, 2))
    for f in range(F):
        n_pos = min(max(int(case['counts'][f, 0]), 0), cap)
        taken = entries(case, f)
        for k, x, y, z, row in taken:
            q[f, k] = q_of_row(reg_row(case, f, x, y, z)[0], case['anchors'][x, y, z], case['gts'][row])
        vals = [q[f, e[0]] for e in taken]
        out[f, 0] = weight / max(1, n_pos) * sum(1.0 - v for v in vals)
        out[f, 1] = sum(vals) / len(vals) if vals else 0.0
    return q, out


def central_differences(case, weight=1.0, h=1e-6):
    """d(sum of the terms)/d(heads) f64 (rows, ld) of restatement (a): seven central differences per entry."""
    F, l, w = case['F'], case['l'], case['w']
    cap = case['gi'].shape[1]
    grad = np.zeros(case['heads'].shape)
    for f in range(F):
        n_pos = min(max(int(case['counts'][f, 0]), 0), cap)
        scale = weight / max(1, n_pos)
        for k, x, y, z, row in entries(case, f):
            r, col = reg_row(case, f, x, y, z)
            an, g = case['anchors'][x, y, z], case['gts'][row]
            if not finite_f32(r, an):
                continue
            r = r.astype(np.float64)
            for c in range(7):
                hi, lo = r.copy(), r.copy()
                hi[c] += h
                lo[c] -= h
                dq = (IR.iou3d(decode64(hi, an), g.astype(np.float64)[:7])[0]
                      - IR.iou3d(decode64(lo, an), g.astype(np.float64)[:7])[0]) / (2 * h)
                grad[(f * l + x) * w + y, col + c] += -scale * dq
    return grad


# ---- (b) ----------------------------------------------------------------------------------------------------------------------
def _f(t):
    return float(t.detach()) if torch.is_tensor(t) else float(t)


def _quad_t(b):
    """BEV corners of a torch box, Calc.bbox3d2bev's formula (clockwise yaw)."""
    c, s = torch.cos(b[6]), torch.sin(b[6])
    pts = []
    for ux, uy in ((0.5, 0.5), (-0.5, 0.5), (-0.5, -0.5), (0.5, -0.5)):
        px, py = ux * b[3], uy * b[4]
        pts.append((px * c + py * s + b[0], -px * s + py * c + b[1]))
    return pts


def _area_t(poly):
    tot = 0.0
    for k in range(len(poly)):
        (x0, y0), (x1, y1) = poly[k], poly[(k + 1) % len(poly)]
        tot = tot + x0 * y1 - y0 * x1
    return 0.5 * tot


def _clip_t(qa, qb):
    """Sutherland-Hodgman over torch scalars: qa clipped by the edges of qb (both counter-clockwise); autograd differentiates
    the vertices it keeps and the crossings it computes."""
    poly = list(qa)
    for i in range(4):
        (ax, ay), (bx, by) = qb[i], qb[(i + 1) % 4]
        side = [(bx - ax) * (py - ay) - (by - ay) * (px - ax) for px, py in poly]
        nxt = []
        for k in range(len(poly)):
            k1 = (k + 1) % len(poly)
            sp, sq = side[k], side[k1]
            if _f(sp) >= 0:
                nxt.append(poly[k])
            if (_f(sp) > 0 and _f(sq) < 0) or (_f(sp) < 0 and _f(sq) > 0):
                t = sp / (sp - sq)
                nxt.append((poly[k][0] + (poly[k1][0] - poly[k][0]) * t, poly[k][1] + (poly[k1][1] - poly[k][1]) * t))
        poly = nxt
        if len(poly) < 3:
            return None
    return _area_t(poly)


def loss_autograd(case, weight=1.0):
    """-> (out f64 (F,2), d(sum_f out[f,0])/d(heads) f64 (rows, ld), q f64 (F,cap))."""
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    cap = case['gi'].shape[1]
    heads = torch.from_numpy(np.asarray(case['heads'], np.float64)).clone().requires_grad_(True)
    anchors = torch.from_numpy(np.asarray(case['anchors'], np.float64))
    gts = torch.from_numpy(np.asarray(case['gts'], np.float64))
    q_out = np.full((F, cap), -1.0)
    terms, means = [], []
    for f in range(F):
        n_pos = min(max(int(case['counts'][f, 0]), 0), cap)
        total, qs = heads.sum() * 0.0, []
        for k, x, y, z, row in entries(case, f):
            r32, col = reg_row(case, f, x, y, z)
            r = heads[(f * l + x) * w + y, col:col + 7]
            an, g = anchors[x, y, z], gts[row]
            q = None
            if finite_f32(r32, case['anchors'][x, y, z]) and bool(torch.isfinite(g[:7]).all()):
                d = torch.sqrt(an[3] ** 2 + an[4] ** 2)
                b = [r[0] * d + an[0], r[1] * d + an[1], r[2] * an[5] + an[2], torch.exp(r[3]) * an[3], torch.exp(r[4]) * an[4],
                     torch.exp(r[5]) * an[5], r[6] + an[6]]
                ih = torch.minimum(b[2] + b[5], g[2] + g[5]) - torch.maximum(b[2], g[2])
                if _f(ih) > 0:
                    qa, qb = _quad_t(b), _quad_t(g)
                    if IR.circle_gap(np.array([[_f(u), _f(v)] for u, v in qa]),
                                     np.array([[_f(u), _f(v)] for u, v in qb])) <= 0:
                        inter = _clip_t(qa, qb)
                        if inter is not None and _f(inter) > 0:
                            vol = inter * ih
                            q = torch.clamp(vol / (b[3] * b[4] * b[5] + g[3] * g[4] * g[5] - vol), 0.0, 1.0)
            if q is None:
                q = heads.sum() * 0.0
            total = total + (1.0 - q)
            qs.append(_f(q))
            q_out[f, k] = _f(q)
        terms.append(weight / max(1, n_pos) * total)
        means.append(sum(qs) / len(qs) if qs else 0.0)
    terms = torch.stack(terms)
    terms.sum().backward()
    return np.stack([terms.detach().numpy(), np.array(means)], axis=1), heads.grad.numpy(), q_out


# ---- the kernel's own algorithm -------------------------------------------------------------------------------------------------
def _clip_pass(poly, side, h, T):
    """One pass of the kernel's clip: poly = [(x, y, tag)], side 0: x <= h, 1: x >= -h, 2: y <= h, 3: y >= -h."""
    def dist(p):
        return (h - p[0], p[0] + h, h - p[1], p[1] + h)[side]
    out = []
    n = len(poly)
    for k in range(n):
        p, q = poly[k], poly[(k + 1) % n]
        dp, dq = dist(p), dist(q)
        pin, qin = dp >= 0, dq >= 0
        if pin and len(out) < 8:
            out.append(p)
        if pin != qin and len(out) < 8:
            u = T(dp / (dp - dq))
            cx, cy = T(p[0] + u * (q[0] - p[0])), T(p[1] + u * (q[1] - p[1]))
            if side == 0:
                cx = h
            elif side == 1:
                cx = T(-h)
            elif side == 2:
                cy = h
            else:
                cy = T(-h)
            out.append((cx, cy, side if pin else p[2]))
    return out


def kernel_entry(r, an, g, T=np.float32):
    """(q, dq/dr (7,)) of one entry by the kernel's algorithm in numpy scalars of type T (operands f32, as on the device)."""
    r, an, g = (np.asarray(v, np.float32).astype(T) for v in (r, an, g))
    zero = np.zeros(7, T)
    half = T(0.5)
    with np.errstate(over='ignore', invalid='ignore'):
        d = T(np.sqrt(T(T(an[3] * an[3]) + T(an[4] * an[4]))))
        b = np.array([T(r[0] * d) + an[0], T(r[1] * d) + an[1], T(r[2] * an[5]) + an[2], T(np.exp(r[3])) * an[3],
                      T(np.exp(r[4])) * an[4], T(np.exp(r[5])) * an[5], r[6] + an[6]], T)
    if not (np.isfinite(b).all() and np.isfinite(g[:7]).all()):
        return T(0), zero
    top_b, top_g = T(b[2] + b[5]), T(g[2] + g[5])
    ih = T(min(top_b, top_g) - max(b[2], g[2]))
    if not ih > 0:
        return T(0), zero
    sb, cb = T(np.sin(b[6])), T(np.cos(b[6]))
    dth = T(g[6] - b[6])
    sd, cd = T(np.sin(dth)), T(np.cos(dth))
    dx, dy = T(g[0] - b[0]), T(g[1] - b[1])
    tx, ty = T(T(cb * dx) - T(sb * dy)), T(T(sb * dx) + T(cb * dy))
    poly = []
    for ux, uy in ((0.5, 0.5), (-0.5, 0.5), (-0.5, -0.5), (0.5, -0.5)):
        px, py = T(T(ux) * g[3]), T(T(uy) * g[4])
        poly.append((T(T(T(px * cd) + T(py * sd)) + tx), T(T(T(px * -sd) + T(py * cd)) + ty), 4))
    hl, hw = T(half * b[3]), T(half * b[4])
    for side, h in ((0, hl), (1, hl), (2, hw), (3, hw)):
        poly = _clip_pass(poly, side, h, T)
    area2 = gtx = gty = gl = gw = gphi = T(0)
    n = len(poly)
    for k in range(n):
        (x0, y0, tag), (x1, y1, _) = poly[k], poly[(k + 1) % n]
        area2 = T(area2 + T(T(x0 * y1) - T(y0 * x1)))
        if tag < 2:
            s, ym = T(abs(T(y1 - y0))), T(half * T(y0 + y1))
            gl = T(gl + T(half * s))
            gtx = T(gtx + (s if tag == 0 else -s))
            gphi = T(gphi + (T(-ym * s) if tag == 0 else T(ym * s)))
        elif tag < 4:
            s, xm = T(abs(T(x1 - x0))), T(half * T(x0 + x1))
            gw = T(gw + T(half * s))
            gty = T(gty + (s if tag == 2 else -s))
            gphi = T(gphi + (T(xm * s) if tag == 2 else T(-xm * s)))
    inter = T(half * area2)
    if n < 3 or not inter > 0:
        return T(0), zero
    vb = T(T(b[3] * b[4]) * b[5])
    vol = T(inter * ih)
    uni = T(T(vb + T(T(g[3] * g[4]) * g[5])) - vol)
    with np.errstate(divide='ignore', invalid='ignore'):
        v = T(vol / uni)
    if not (np.isfinite(v) and uni > 0):
        return T(0), zero
    q = T(min(max(v, T(0)), T(1)))
    dI = (T(T(cb * gtx) + T(sb * gty)), T(T(-sb * gtx) + T(cb * gty)), T(0), gl, gw, T(0), T(-gphi))
    lower = T(1) if top_b < top_g else T(0)
    dih = (T(0), T(0), T(lower - (T(1) if b[2] > g[2] else T(0))), T(0), T(0), lower, T(0))
    dvb = (T(0), T(0), T(0), T(b[4] * b[5]), T(b[3] * b[5]), T(b[3] * b[4]), T(0))
    chain = (d, d, an[5], b[3], b[4], b[5], T(1))
    inv_u2 = T(T(1) / T(uni * uni))
    grad = np.zeros(7, T)
    for c in range(7):
        dV = T(T(ih * dI[c]) + T(inter * dih[c]))
        dq = T(T(T(dV * T(uni + vol)) - T(vol * dvb[c])) * inv_u2)
        grad[c] = T(dq * chain[c])
    return q, grad


def kernel_restated(case, weight=1.0, T=np.float32):
    """-> (q (F,cap), out (F,2) f64, d_heads (rows, ld) of type T): the kernel's arithmetic entry by entry, the gradient of
    entries that share an anchor added in list order."""
    F, l, w = case['F'], case['l'], case['w']
    cap = case['gi'].shape[1]
    q = np.full((F, cap), -1.0)
    out = np.zeros((F, 2))
    grad = np.zeros(case['heads'].shape, T)
    for f in range(F):
        n_pos = min(max(int(case['counts'][f, 0]), 0), cap)
        scale = T(T(weight) / T(max(1, n_pos)))
        taken = entries(case, f)
        for k, x, y, z, row in taken:
            r, col = reg_row(case, f, x, y, z)
            val, dq = kernel_entry(r, case['anchors'][x, y, z], case['gts'][row, :7], T)
            q[f, k] = float(val)
            for c in range(7):
                grad[(f * l + x) * w + y, col + c] += T(T(-scale * dq[c]))
        vals = [q[f, e[0]] for e in taken]
        out[f, 0] = float(weight) / max(1, n_pos) * sum(1.0 - v for v in vals)
        out[f, 1] = sum(vals) / len(vals) if vals else 0.0
    return q, out, grad
