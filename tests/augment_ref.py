"""Host restatement of the GT-paste augmentation's contract (include/mvx_hip.h "GT-paste augmentation"), in numpy,
used by the augmentation tests as tests/detect_ref.py is used by the detection tests.  float64 where the contract says
float64 (the ground grid's cell index), float32 where it says float32 (the candidate's cell, the 2-D ratio, the comparisons);
sequential, slot by slot and candidate by candidate; the rotated IoU comes from the C oracle (mvx_oracle.bbox_pairwise,
candidate against scene box)."""
import numpy as np

F32 = np.float32


def ground_grid(pcd, velorange, gridshape=(704, 800)):
    """zmax f32 (gh, gw): largest z per cell, f32(velorange[2] - 1) where empty; points outside the x/y range (or with a NaN
    z) are skipped; -0 counts as +0."""
    pcd = np.asarray(pcd, np.float32)
    gh, gw = gridshape
    lo = np.array(velorange[:2], np.float64)
    hi = np.array(velorange[3:5], np.float64)
    size = np.array([(velorange[3] - velorange[0]) / gh, (velorange[4] - velorange[1]) / gw])
    zmax = np.full((gh, gw), F32(velorange[2] - 1), np.float32)
    xy = pcd[:, :2].astype(np.float64)
    ok = np.all((xy >= lo) & (xy < hi), axis=1) & ~np.isnan(pcd[:, 2])
    loc = ((xy[ok] - lo) / size).astype(np.int32)
    z = pcd[ok, 2] + F32(0)                                         # -0 + 0 = +0
    inside = (loc[:, 0] >= 0) & (loc[:, 0] < gh) & (loc[:, 1] >= 0) & (loc[:, 1] < gw)
    np.maximum.at(zmax, (loc[inside, 0], loc[inside, 1]), z[inside])
    return zmax


def iof_f32(scene2d, gt2d):
    """inter(scene_i, gt) / area(scene_i), all float32 (utils/Bbox.py + box_area)."""
    s, g = np.asarray(scene2d, np.float32), np.asarray(gt2d, np.float32)
    w = np.maximum(np.minimum(s[:, 2], g[2]) - np.maximum(s[:, 0], g[0]), F32(0))
    h = np.maximum(np.minimum(s[:, 3], g[3]) - np.maximum(s[:, 1], g[1]), F32(0))
    area = (s[:, 2] - s[:, 0]) * (s[:, 3] - s[:, 1])
    with np.errstate(divide='ignore', invalid='ignore'):
        return (w * h) / area


def candidate_cell(b3, velorange, cell=0.1):
    """(gx, gy) of a candidate's centre in float32 with a true division, or None when outside the grid's index range."""
    qx = (F32(b3[0]) - F32(velorange[0])) / F32(cell)
    qy = (F32(b3[1]) - F32(velorange[1])) / F32(cell)
    return qx, qy


def place_frame(zmax, velorange, box2d, box3d, bev, lim, cand, thr, db, iou_fn, cell=0.1, z_margin=0.1, iou_thr=0.05):
    """One frame.  box2d (n,4), box3d (n,7), bev (n,4,2) f32; cand i32 (S, C) database indices (-1 = none), thr f32 (S,);
    db = dict(box2d, box3d, bev) numpy f32 tables.  Returns dict(picked (S,), fail (S, C), val (S, C, 3), box2d, box3d,
    bev): fail = first failing test 0 ground / 1 2-D / 2 BEV, 3 = passes, -1 = no candidate or slot not run."""
    gh, gw = zmax.shape
    b2, b3, bv = [np.asarray(a, np.float32).copy() for a in (box2d, box3d, bev)]
    b2, b3, bv = b2.reshape(-1, 4), b3.reshape(-1, 7), bv.reshape(-1, 4, 2)
    n0 = b3.shape[0]
    S_all, C = cand.shape
    picked = np.full((S_all,), -1, np.int32)
    fail = np.full((S_all, C), -1, np.int32)
    val = np.zeros((S_all, C, 3), np.float32)
    S = 0 if n0 > lim else lim - n0
    assert S <= S_all
    for s in range(S):
        n = b3.shape[0]
        win = -1
        for c in range(C):
            idx = int(cand[s, c])
            if idx < 0 or idx >= db['box3d'].shape[0]:
                continue
            g3, g2, gb = db['box3d'][idx], db['box2d'][idx], db['bev'][idx]
            qx, qy = candidate_cell(g3, velorange, cell)
            ground_ok = False
            zg = F32(0)
            if qx > F32(-1) and qx < F32(gh) and qy > F32(-1) and qy < F32(gw):
                zg = zmax[int(qx), int(qy)]
                ground_ok = not (zg > F32(g3[2]) + F32(z_margin))
            m_iof = m_iou = F32(0)
            if n > 0:
                m_iof = np.fmax.reduce(np.concatenate([[F32(-np.inf)], iof_f32(b2, g2)])).astype(np.float32)
                m_iou = np.fmax.reduce(np.concatenate([[F32(-np.inf)], iou_fn(gb[None], bv)[0]])).astype(np.float32)
            val[s, c] = (zg, m_iof, m_iou)
            f = 0 if not ground_ok else 1 if (n > 0 and m_iof > F32(thr[s])) else 2 if (n > 0 and m_iou > F32(iou_thr)) else 3
            fail[s, c] = f
            if f == 3 and win < 0:
                win = c
        if win >= 0:
            idx = int(cand[s, win])
            picked[s] = idx
            b2 = np.concatenate([b2, db['box2d'][idx][None]], 0)
            b3 = np.concatenate([b3, db['box3d'][idx][None]], 0)
            bv = np.concatenate([bv, db['bev'][idx][None]], 0)
    return dict(picked=picked, fail=fail, val=val, box2d=b2, box3d=b3, bev=bv)


def paste_points(pcd6, picked, db_points, pt_off, cap):
    """Scene rows (n,6) plus the picked objects' rows in slot order; an object that does not fit ``cap`` is dropped whole.
    Returns (rows, overflow flag)."""
    out = [np.asarray(pcd6, np.float32)]
    n = out[0].shape[0]
    overflow = False
    for idx in picked:
        if idx < 0:
            continue
        rows = db_points[pt_off[idx]:pt_off[idx + 1]]
        if n + rows.shape[0] > cap:
            overflow = True
            continue
        out.append(rows)
        n += rows.shape[0]
    return np.concatenate(out, 0), overflow


def paste_image(img, picked, patch, mask, px_off, maskbbox):
    """img u8 (H,W,3) copy with every picked object's patch under its mask, in slot order, clipped to the image."""
    img = np.array(img, np.uint8)
    H, W = img.shape[:2]
    for idx in picked:
        if idx < 0:
            continue
        x1, y1, x2, y2 = (int(v) for v in maskbbox[idx])
        w, h = x2 - x1 + 1, y2 - y1 + 1
        if w <= 0 or h <= 0:
            continue
        p = patch[px_off[idx]:px_off[idx + 1]].reshape(h, w, 3)
        m = mask[px_off[idx]:px_off[idx + 1]].reshape(h, w) != 0
        ys, xs = np.nonzero(m)
        ok = (ys + y1 >= 0) & (ys + y1 < H) & (xs + x1 >= 0) & (xs + x1 < W)
        img[ys[ok] + y1, xs[ok] + x1] = p[ys[ok], xs[ok]]
    return img


def db_tables(db):
    """numpy copies of a LoadGT.GTDatabase's tables."""
    return {k: getattr(db, k).cpu().numpy() for k in ('box2d', 'box3d', 'bev', 'points', 'pt_off', 'patch', 'mask', 'px_off',
                                                      'maskbbox')}
