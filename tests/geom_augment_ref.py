"""Host restatement of the geometric augmentation's contract (include/mvx_hip.h "Geometric augmentation") in
float64 numpy with sequential loops; imports nothing of the package.  The BEV IoU is handed in (``iou(a, b) -> (N, M)``: the
tests pass ``mvx_oracle.bbox_pairwise``), as tests/augment_ref.py takes it.

Decisions are thresholds on computed values, so ``place_frame`` asserts that no IoU it compares lies within IOU_BAND of the
threshold and ``clean_cloud`` removes from an INPUT cloud the points whose membership or range values lie within FACE_BAND of a
box face or a range face; nothing is left out of a comparison afterwards."""
import numpy as np

IOU_BAND = 1e-5          # the paste test's band
FACE_BAND = 1e-3         # metres


def rot(p, a):
    """p @ R(a), R(a) = [[cos a, -sin a], [sin a, cos a]] (Calc.getRotationMatrices) on row vectors."""
    p = np.asarray(p, np.float64)
    c, s = np.cos(a), np.sin(a)
    return np.stack([p[..., 0] * c + p[..., 1] * s, -p[..., 0] * s + p[..., 1] * c], -1)


def quad(box):
    """Calc.bbox3d2bev of one box x y z l w h r: (4, 2) float64."""
    b = np.asarray(box, np.float64)
    local = np.array([[0.5, 0.5], [-0.5, 0.5], [-0.5, -0.5], [0.5, -0.5]]) * b[3:5]
    return rot(local, b[6]) + b[:2]


def wrap(r):
    return r - 2.0 * np.pi * np.floor((r + np.pi) / (2.0 * np.pi))


def place_frame(boxes, noise, iou_thr, iou, check_band=True):
    """Boxes (n, 7) in index order, noise (>= n, T, 4).  Returns (trial (n,) int, move (n, 4), moved boxes (n, 7), the IoUs
    that were compared (list of arrays))."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
    n = boxes.shape[0]
    T = noise.shape[1]
    quads = [quad(b) for b in boxes]
    trial = np.full((n,), -1, np.int64)
    move = np.zeros((n, 4))
    moved = boxes.copy()
    seen = []
    for i in range(n):
        others = [j for j in range(n) if j != i]
        for t in range(T):
            d = np.asarray(noise[i, t], np.float64)
            cand = boxes[i].copy()
            cand[0] += d[0]
            cand[1] += d[1]
            cand[6] += d[3]
            q = quad(cand)
            ok = True
            if others:
                v = iou(q[None].astype(np.float32), np.stack([quads[j] for j in others]).astype(np.float32))[0].astype(np.float64)
                seen.append(v)
                if check_band:
                    assert (np.abs(v - iou_thr) > IOU_BAND).all(), (i, t, v)
                ok = not (v.max() > iou_thr)
            if ok:
                trial[i] = t
                move[i] = d
                quads[i] = q
                moved[i, 0] += d[0]
                moved[i, 1] += d[1]
                moved[i, 2] += d[2]
                moved[i, 6] += d[3]
                break
    return trial, move, moved, seen


def owner_of(boxes, pts):
    """Lowest index of the box each point lies in (-1 none) and the smallest distance of a membership value to a face."""
    pts = np.asarray(pts, np.float64)
    own = np.full((pts.shape[0],), -1, np.int64)
    margin = np.full((pts.shape[0],), np.inf)
    for i in range(np.asarray(boxes).reshape(-1, 7).shape[0] - 1, -1, -1):
        b = np.asarray(boxes[i], np.float64)
        dx, dy, dz = pts[:, 0] - b[0], pts[:, 1] - b[1], pts[:, 2] - b[2]
        c, s = np.cos(b[6]), np.sin(b[6])
        u, v = dx * c - dy * s, dx * s + dy * c
        inside = (np.abs(u) <= b[3] / 2) & (np.abs(v) <= b[4] / 2) & (dz >= 0) & (dz <= b[5])
        own[inside] = i
        m = np.minimum.reduce([np.abs(np.abs(u) - b[3] / 2), np.abs(np.abs(v) - b[4] / 2), np.abs(dz), np.abs(dz - b[5])])
        margin = np.minimum(margin, m)
    return own, margin


def global_points(xyz, glob):
    phi, s, flip = float(glob[0]), float(glob[1]), bool(glob[2])
    out = np.empty_like(xyz)
    out[:, :2] = s * rot(xyz[:, :2], phi)
    out[:, 2] = s * xyz[:, 2]
    if flip:
        out[:, 1] = -out[:, 1]
    return out


def object_points(pts, boxes, trial, move):
    """The per-object step on (P, >= 3) points: float64 x y z."""
    xyz = np.asarray(pts, np.float64)[:, :3].copy()
    boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
    own, _ = owner_of(boxes, xyz)
    for k in range(xyz.shape[0]):
        i = own[k]
        if i >= 0 and trial[i] >= 0:
            c = boxes[i, :2]
            xyz[k, :2] = rot(xyz[k, :2] - c, move[i, 3]) + c + move[i, :2]
            xyz[k, 2] += move[i, 2]
    return xyz, own


def transform_points(pts, boxes, trial, move, glob):
    xyz, own = object_points(pts, boxes, trial, move)
    return global_points(xyz, glob), own


def in_range(xyz, velorange):
    lo, hi = np.asarray(velorange[:3], np.float64), np.asarray(velorange[3:], np.float64)
    return ((xyz >= lo) & (xyz < hi)).all(1)


def range_margin(xyz, velorange):
    lo, hi = np.asarray(velorange[:3], np.float64), np.asarray(velorange[3:], np.float64)
    return np.minimum(np.abs(xyz - lo), np.abs(xyz - hi)).min(1)


def global_boxes(moved, glob):
    phi, s, flip = float(glob[0]), float(glob[1]), bool(glob[2])
    out = np.asarray(moved, np.float64).reshape(-1, 7).copy()
    out[:, :3] = global_points(out[:, :3].copy(), glob)
    out[:, 3:6] *= s
    r = out[:, 6] + phi
    out[:, 6] = wrap(-r if flip else r)
    return out


def augment_frame(pts6, boxes, noise, glob, velorange, iou_thr, iou, check_band=True):
    """One frame.  pts6 (P, 6) f32, boxes (n, 7) f32.  Returns a dict: trial, move, kept_boxes (indices), box3d (k, 7), bev
    (k, 4, 2), kept_points (indices, in order), xyz (their float64 coordinates), rest (columns 3..5 of the kept rows, untouched)."""
    pts6 = np.asarray(pts6)
    boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
    trial, move, moved, _ = place_frame(boxes, noise, iou_thr, iou, check_band)
    out_b = global_boxes(moved, glob)
    lo, hi = np.asarray(velorange[:2], np.float64), np.asarray(velorange[3:5], np.float64)
    keep_b = ((out_b[:, :2] >= lo) & (out_b[:, :2] < hi)).all(1)
    if check_band and out_b.shape[0]:
        assert (np.minimum(np.abs(out_b[:, :2] - lo), np.abs(out_b[:, :2] - hi)) > FACE_BAND).all()
    xyz, own = transform_points(pts6, boxes, trial, move, glob)
    keep_p = in_range(xyz, velorange) if xyz.shape[0] else np.zeros((0,), bool)
    if check_band and xyz.shape[0]:
        finite = np.isfinite(xyz).all(1)
        assert (range_margin(xyz[finite], velorange) > FACE_BAND * 0.999).all()
        if boxes.shape[0]:
            assert (owner_of(boxes, np.asarray(pts6, np.float64)[finite, :3])[1] > FACE_BAND * 0.999).all()
    kb = np.nonzero(keep_b)[0]
    kp = np.nonzero(keep_p)[0]
    return dict(trial=trial, move=move, kept_boxes=kb, box3d=out_b[kb], bev=np.stack([quad(b) for b in out_b[kb]]) if kb.size else
                np.zeros((0, 4, 2)), kept_points=kp, xyz=xyz[kp], rest=pts6[kp, 3:], owner=own)


def clean_cloud(pts6, boxes, noise, glob, velorange, iou_thr, iou):
    """The rows of an input cloud whose float64 membership and range values are FACE_BAND away from every face."""
    pts6 = np.asarray(pts6)
    if pts6.shape[0] == 0:
        return pts6
    boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
    trial, move, _, _ = place_frame(boxes, noise, iou_thr, iou, check_band=False)
    xyz, _ = transform_points(pts6, boxes, trial, move, glob)
    ok = range_margin(xyz, velorange) > FACE_BAND
    if boxes.shape[0]:
        ok &= owner_of(boxes, np.asarray(pts6, np.float64)[:, :3])[1] > FACE_BAND
    return pts6[ok]


def draw_like(F, B, T, rng, rot_obj=np.pi / 10, sigma=(1.0, 1.0, 1.0), scale=(0.95, 1.05), rot_glob=np.pi / 4, flip_p=0.5):
    """Geometry.draw_geometry's order of draws, restated."""
    noise = np.empty((F, B, T, 4), np.float32)
    noise[..., :3] = rng.normal(0.0, 1.0, (F, B, T, 3)) * np.asarray(sigma)
    noise[..., 3] = rng.uniform(-rot_obj, rot_obj, (F, B, T))
    glob = np.zeros((F, 4), np.float32)
    glob[:, 0] = rng.uniform(-rot_glob, rot_glob, F)
    glob[:, 1] = rng.uniform(scale[0], scale[1], F)
    glob[:, 2] = rng.random(F) < flip_p
    return noise, glob
