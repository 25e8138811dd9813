"""References of the ignore pass (csrc/ignore.hip) for tests/test_ignore_host.py and tests/test_ignore_gpu.py.

ignore_rule: the rule of one frame restated in numpy on dense inputs -- the lists of the assigner, the point count of every box,
the projected anchor centres (``project``, float64 in the operand order of the header), the rectangles, and the (B, N) table of
intersections of the ignore quads with the anchors plus the anchors' f32 shoelace areas (``area32``).  No geometry is clipped
here: the GPU tests take the table from mvx_bbox_pairwise(.., 0) of the same run.
point_counts64: the points inside every box in float64 (box3d.h's ``inside``), with the distance of the nearest point from a
face so that a fixture can show that no decision is a rounding question."""
import numpy as np


def project(anchors7, matrix):
    """anchors7 (N, 7) f32, matrix (3, 4) f64 -> (px, py, depth), each (N,) f64: the centre (x, y, z + h/2, 1) through the matrix
    as ((m0 x + m1 y) + m2 zc) + m3, every product and sum rounded on its own."""
    a = np.asarray(anchors7, np.float32).astype(np.float64).reshape(-1, 7)
    m = np.asarray(matrix, np.float64).reshape(3, 4)
    x, y, zc = a[:, 0], a[:, 1], a[:, 2] + a[:, 5] / 2.0
    rows = [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * zc) + m[r, 3] for r in range(3)]
    d = rows[2]
    front = d > 0.0
    safe = np.where(front, d, 1.0)
    return np.where(front, rows[0] / safe, np.nan), np.where(front, rows[1] / safe, np.nan), d


def in_rects(px, py, depth, rects):
    """(N,) bool: depth > 0 and the pixel inside one of rects (R, 4) = (x1, y1, x2, y2), edges inclusive; and the smallest
    distance (px) of a centre in front of the camera from an edge line it could cross."""
    rects = np.asarray(rects, np.float32).astype(np.float64).reshape(-1, 4)
    hit = np.zeros(px.shape, bool)
    margin = np.inf
    front = depth > 0.0
    for x1, y1, x2, y2 in rects:
        with np.errstate(invalid='ignore'):
            inside = front & (px >= x1) & (px <= x2) & (py >= y1) & (py <= y2)
        hit |= inside
        if front.any():
            dx = np.minimum(np.abs(px[front] - x1), np.abs(px[front] - x2))
            dy = np.minimum(np.abs(py[front] - y1), np.abs(py[front] - y2))
            near_x = (py[front] >= y1 - 1.0) & (py[front] <= y2 + 1.0)          # an x edge matters only beside the rectangle
            near_y = (px[front] >= x1 - 1.0) & (px[front] <= x2 + 1.0)
            for d, near in ((dx, near_x), (dy, near_y)):
                if near.any():
                    margin = min(margin, float(d[near].min()))
    return hit, margin


def area32(quads):
    """|shoelace| of quads (N, 4, 2) in f32 exactly as bev_iou.h's shoelace: products, differences and the running sum in f32 in
    corner order, the halving in f64, rounded to f32."""
    q = np.asarray(quads, np.float32).reshape(-1, 4, 2)
    acc = np.zeros((q.shape[0],), np.float32)
    for k in range(4):
        u, v = q[:, k], q[:, (k + 1) % 4]
        acc = (acc + ((u[:, 0] * v[:, 1]).astype(np.float32) - (u[:, 1] * v[:, 0]).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return np.abs((acc.astype(np.float64) / 2.0).astype(np.float32))


def ignore_rule(n_anchors, pos, gi, notneg, gt_points=None, min_points=0, centres=None, rects=None, inter=None, area=None, ioa_thr=0.5):
    """One frame.  pos / notneg: flat anchor indices of the incoming lists, gi the box of every positive; gt_points (G,) or None;
    centres = (px, py, depth) of ``project`` with rects (R, 4), or None; inter (B, N) f32 with area (N,) f32, or None.
    Returns dict(pos, gi, notneg: the rewritten lists, ascending; stats: [demoted, by a rectangle, by a box only, sparse boxes])."""
    pos, gi, notneg = (np.asarray(v, np.int64) for v in (pos, gi, notneg))
    is_pos = np.zeros((n_anchors,), bool)
    match = np.full((n_anchors,), -1, np.int64)
    nn = np.zeros((n_anchors,), bool)
    nn[notneg] = True
    sparse = np.zeros((0,), bool)
    if gt_points is not None:
        sparse = np.asarray(gt_points) < min_points
    demoted = 0
    for a, g in zip(pos, gi):
        nn[a] = True
        if gt_points is not None and g < len(sparse) and sparse[g]:
            demoted += 1
            continue
        is_pos[a] = True
        match[a] = g
    by_rect = np.zeros((n_anchors,), bool)
    if centres is not None and rects is not None and len(rects):
        by_rect = in_rects(centres[0], centres[1], centres[2], rects)[0] & ~nn
    nn |= by_rect
    by_box = np.zeros((n_anchors,), bool)
    if inter is not None and len(inter):
        inter = np.asarray(inter, np.float32)
        bound = (np.float32(ioa_thr) * np.asarray(area, np.float32)).astype(np.float32)
        by_box = (inter >= bound[None]).any(axis=0) & ~nn
    nn |= by_box
    p = np.flatnonzero(is_pos)
    return dict(pos=p, gi=match[p], notneg=np.flatnonzero(nn), stats=[demoted, int(by_rect.sum()), int(by_box.sum()), int(sparse.sum())])


def box_margin(inter, area, ioa_thr):
    """Smallest |inter - ioa_thr * area| / area over the pairs with a non-zero intersection (inf when there is none)."""
    inter = np.asarray(inter, np.float64)
    area = np.asarray(area, np.float64)[None]
    d = np.abs(inter - ioa_thr * area) / area
    d = d[inter > 0]
    return float(d.min()) if d.size else np.inf


def point_counts64(points, n_points, boxes, gt_off):
    """points (F, cap, ld) f32, n_points (F,), boxes (G, 7) f32 xyzlwhr (z = bottom face), gt_off (F+1,) -> (counts i32 (G,), the
    smallest distance (m) of a counted or uncounted point from a face of a box it lies beside)."""
    points = np.asarray(points, np.float32)
    boxes = np.asarray(boxes, np.float32).astype(np.float64).reshape(-1, 7)
    counts = np.zeros((boxes.shape[0],), np.int32)
    margin = np.inf
    for f in range(points.shape[0]):
        p = points[f, :int(n_points[f]), :3].astype(np.float64)
        for g in range(int(gt_off[f]), int(gt_off[f + 1])):
            b = boxes[g]
            c, s = np.cos(b[6]), np.sin(b[6])
            dx, dy, dz = p[:, 0] - b[0], p[:, 1] - b[1], p[:, 2] - b[2]
            u, v = dx * c - dy * s, dx * s + dy * c
            inside = (np.abs(u) <= b[3] / 2.0) & (np.abs(v) <= b[4] / 2.0) & (dz >= 0.0) & (dz <= b[5])
            counts[g] = inside.sum()
            if p.shape[0]:
                faces = np.stack([np.abs(np.abs(u) - b[3] / 2.0), np.abs(np.abs(v) - b[4] / 2.0), np.abs(dz), np.abs(dz - b[5])])
                near = (np.abs(u) <= b[3] / 2.0 + 0.01) & (np.abs(v) <= b[4] / 2.0 + 0.01) & (dz >= -0.01) & (dz <= b[5] + 0.01)
                if near.any():
                    margin = min(margin, float(faces[:, near].min()))
    return counts, margin
