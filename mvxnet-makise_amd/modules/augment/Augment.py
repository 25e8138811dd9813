"""GT-paste augmentation with the reference's names (modules/augment/Augment.py), decided on the GPU (csrc/augment.hip).

The host draws the random numbers -- per slot 30 database objects without replacement, then one of the three 2-D overlap
thresholds, from ``np.random`` in the reference's order (both are drawn before any test, so the draws do not depend on the
outcomes) -- and the kernels do the rest: the ground grid of the scene cloud, the sequential placement of the slots, the
paste of the picked objects' points behind the scene points and of their image patches under their masks.

``augmentTargetClasses`` / ``augment`` / ``locate`` / ``check`` keep the reference's signatures and return values and run the
single-frame case; ``augmentFrames`` is the frame-set form for the frames of a step (four launches, one host read)."""

import numpy as np
import torch

import modules.config as cfg
from modules import _hip
from modules import Extension as X
from modules.augment.LoadGT import GTDatabase

IOF_THRS = (0.1, 0.3, 0.5)
ITERLIM = 30
BEV_IOU_THR = 0.05
GRIDSHAPE = (704, 800)
_DB_CACHE = {}


def database_of(gts, device=None):
    """The packed tables of a list of objects as ``LoadGT.getAllGT`` returns it (built once per list and kept)."""
    if isinstance(gts, GTDatabase):
        return gts
    dev = X.device() if device is None else torch.device(device)
    hit = _DB_CACHE.get(id(gts))
    if hit is None or hit[0] is not gts or hit[1].device != dev or hit[1].n != len(gts):
        hit = (gts, GTDatabase.from_gts(gts, dev))
        _DB_CACHE.clear()
        _DB_CACHE[id(gts)] = hit
    return hit[1]


def draw_slots(n_db, n_slots, iterlim=ITERLIM, rng=None):
    """(cand i32 (n_slots, iterlim), thr f32 (n_slots,)): per slot ``min(iterlim, n_db)`` objects without replacement (-1
    padded), then the threshold.  ``rng=None`` draws from ``np.random`` exactly as the reference's ``locate`` does
    (``np.random.choice(gts, 30, replace=False)`` consumes the stream like the same call on ``len(gts)``: a full
    permutation of the database per slot); a ``np.random.Generator`` draws the same distribution without the permutation."""
    k = min(iterlim, n_db)
    cand = np.full((n_slots, iterlim), -1, np.int32)
    thr = np.zeros((n_slots,), np.float32)
    for s in range(n_slots):
        if rng is None:
            cand[s, :k] = np.random.choice(n_db, k, replace=False)
            thr[s] = np.random.choice(IOF_THRS)
        else:
            cand[s, :k] = rng.choice(n_db, k, replace=False)
            thr[s] = rng.choice(IOF_THRS)
    return cand, thr


def _points6(pcd, dev):
    p = np.ascontiguousarray(np.asarray(pcd)[:, :3], dtype=np.float32)
    t = torch.zeros((1, max(1, p.shape[0]), 6), dtype=torch.float32, device=dev)
    t[0, :p.shape[0], :3] = torch.from_numpy(p).to(dev)
    return t, torch.tensor([p.shape[0]], dtype=torch.int32, device=dev)


def check(pcd, velorange, gridshape=GRIDSHAPE):
    """Largest point z per x/y cell, (gridshape) float64, ``velorange[2] - 1`` where a cell is empty (Augment.py:12-22)."""
    dev = X.device()
    pts, n = _points6(pcd, dev)
    return _hip.gt_paste_ground(pts, n, velorange, gridshape)[0].cpu().numpy().astype(np.float64)


def _scene_tables(scenes, cap, dev):
    """Per-frame (bbox2d, bbox3d, bev) or None -> padded host tables and counts."""
    F = len(scenes)
    b2, b3, bv = torch.zeros((F, cap, 4)), torch.zeros((F, cap, 7)), torch.zeros((F, cap, 4, 2))
    n = torch.zeros((F,), dtype=torch.int32)
    for f, sc in enumerate(scenes):
        if sc is None or sc[1] is None or sc[1].shape[0] == 0:
            continue
        k = sc[1].shape[0]
        if k > cap:
            raise X.MvxHipError('a frame holds %d boxes, the placement takes at most %d' % (k, cap))
        b2[f, :k], b3[f, :k], bv[f, :k] = sc[0].detach().float().cpu(), sc[1].detach().float().cpu()[:, :7], sc[2].detach().float().cpu()
        n[f] = k
    return b2.to(dev), b3.to(dev), bv.to(dev), n


def _raise_on(status):
    bad = 0
    for s in status:
        bad |= int(s)
    if bad & ~_hip.GT_PASTE_POINTS_OVERFLOW:
        raise X.MvxHipError('GT paste: status %d (2 = box count outside the table, 4 = too few slots drawn, 8 = a candidate index '
                            'outside the database)' % bad)
    return bad


def _run_single(pcd, img, b2, b3, bv, db, lim, cand, thr):
    """One frame through ground + placement (+ image paste): (picked list, bbox3d, bev, bbox2d, img)."""
    dev = db.device
    n0 = 0 if b3 is None else b3.shape[0]
    cap = _hip.GT_PASTE_MAX_BOXES
    t2, t3, tv, n = _scene_tables([None if n0 == 0 else (b2, b3, bv)], cap, dev)
    pts, npts = _points6(pcd, dev)
    zmax = _hip.gt_paste_ground(pts, npts, cfg.velorange, GRIDSHAPE)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    picked, n_out = _hip.gt_paste_place(zmax, cfg.velorange, t2, t3, tv, n.to(dev), lim, torch.from_numpy(cand[None]).to(dev),
                                        torch.from_numpy(thr[None]).to(dev), db, status, iou_thr=BEV_IOU_THR)
    img_dev = None
    if img is not None:
        img_dev = _hip.gt_paste_image(torch.from_numpy(np.ascontiguousarray(img, dtype=np.uint8)[None]).to(dev), picked, db)
    host = torch.cat([picked.reshape(-1), n_out, status]).tolist()          # the one host read
    _raise_on(host[-1:])
    k = host[-2]
    out_img = img_dev[0].cpu().numpy() if img_dev is not None else None
    return [p for p in host[:-2] if p >= 0], t3[0, :k].cpu(), tv[0, :k].cpu(), t2[0, :k].cpu(), out_img


def locate(scenepcd, scenebevs, scenebbox2ds, scenebbox3ds, gts, iterlim=ITERLIM):
    """One slot (Augment.py:27-60): the first of ``iterlim`` drawn objects that passes the ground, 2-D and BEV tests, with
    its 'bev' set, or None."""
    db = database_of(gts)
    cand, thr = draw_slots(db.n, 1, iterlim)
    n0 = scenebbox3ds.shape[0]
    picked, _, bev, _, _ = _run_single(scenepcd, None, scenebbox2ds, scenebbox3ds, scenebevs, db, n0 + 1, cand, thr)
    if not picked:
        return None
    gt = db.gts[picked[0]]
    gt['bev'] = bev[-1]
    return gt


def augment(pcd, img, scenebbox2ds, scenebbox3ds, scenebevs, gts, lim):
    """Augment.py:62-90: up to ``lim - n_scene`` objects pasted.  Returns (their clouds, their calibrations, the pasted
    image copy, all 3-D boxes, all bevs)."""
    if scenebbox2ds is None:
        scenebbox2ds, scenebbox3ds, scenebevs = torch.empty((0, 4)), torch.empty((0, 7)), torch.empty((0, 4, 2))
    n0 = scenebbox3ds.shape[0]
    if lim < n0:
        return [], [], img, scenebbox3ds, scenebevs
    db = database_of(gts)
    if lim == n0:
        return [], [], img.copy(), scenebbox3ds, scenebevs
    cand, thr = draw_slots(db.n, lim - n0)
    picked, b3, bv, _, out = _run_single(pcd, img, scenebbox2ds, scenebbox3ds, scenebevs, db, lim, cand, thr)
    return [db.velo_kept[p] for p in picked], [db.gts[p]['calib'] for p in picked], out, b3, bv


def augmentTargetClasses(pcd, img, bbox2ds, bbox3ds, bevs, gtwithinfo, targets, lims):
    """Augment.py:92-114: ``augment`` per target class.  Returns (clouds to add, their calibrations, the image after the
    paste, {class: all 3-D boxes}, {class: all bevs})."""
    augvelos, augcalibs, augbbox3ds, augbevs = [], [], {}, {}
    for c, l in zip(targets, lims):
        velo, calib, img, b3, bv = augment(pcd, img, bbox2ds, bbox3ds, bevs, gtwithinfo[c], l)
        augvelos.extend(velo)
        augcalibs.extend(calib)
        augbbox3ds[c], augbevs[c] = b3, bv
    return augvelos, augcalibs, img, augbbox3ds, augbevs


class FramesResult:
    """What ``augmentFrames`` leaves: ``boxes`` per frame ``(bev (n,4,2), centres (n,2))`` or None, as
    Calc.classifyAnchorsFrames takes them; ``bbox3d`` per frame (n,7) on the device or None; ``picked`` per frame the pasted
    database indices in slot order; ``n_points`` the new point counts (host list); ``status`` per frame.  With the geometric
    augmentation ``boxes`` / ``bbox3d`` / ``n_points`` are those behind it, ``bbox2d`` is None (the 2-D boxes are stale) and
    ``geometry`` holds its Geometry.GeomResult (None otherwise)."""
    __slots__ = ('boxes', 'bbox3d', 'bbox2d', 'picked', 'n_points', 'status', 'debug', 'geometry')


def augmentFrames(batch, images, scene_boxes, db, lim=12, cand=None, thr=None, rng=None, debug=False, shuffle=True, geometry=None):
    """GT paste for the frames of ``batch`` (pipeline.FrameBatch with prepared ``points6`` / ``n_points``) in four launches.
    ``images``: u8 device tensor (F, H, W, 3) pasted in place, or None; ``scene_boxes``: per frame (bbox2d, bbox3d, bev) or
    None; ``db``: GTDatabase on the batch's device.  ``cand`` i32 (F, S, 30) / ``thr`` f32 (F, S): the draws, made here when
    None -- from ``np.random`` in the reference's order (frame by frame, slot by slot), or from the Generator ``rng``.
    The points go behind each frame's scene points, ``batch.n_points`` is replaced, and -- after the ONE host read of the
    call (picked, box counts, point counts, status) -- the shuffle permutations of scene plus pasted points are drawn
    into ``batch.perms`` (``shuffle``; the permutation stays an input of the voxelizer).
    ``geometry`` (default None: off): a Geometry.GeomParams or a dict as Geometry.geometry_draws takes it -- the geometric
    augmentation's launches then go behind the point paste, on scene plus pasted boxes and points, and its words ride in the
    same host read; the paste's own decisions do not depend on it."""
    dev = batch.device
    F = batch.n_frames
    cap = _hip.GT_PASTE_MAX_BOXES
    if lim > cap:
        raise X.MvxHipError('lim is at most %d' % cap)
    b2, b3, bv, n_host = _scene_tables(scene_boxes, cap, dev)
    slots = [max(0, lim - int(k)) if int(k) <= lim else 0 for k in n_host]
    if cand is None:
        S = max(1, max(slots))
        cand = np.full((F, S, ITERLIM), -1, np.int32)
        thr = np.zeros((F, S), np.float32)
        for f in range(F):
            cand[f, :slots[f]], thr[f, :slots[f]] = draw_slots(db.n, slots[f], ITERLIM, rng)
    cand_d = torch.as_tensor(np.ascontiguousarray(cand, dtype=np.int32)).to(dev)
    thr_d = torch.as_tensor(np.ascontiguousarray(thr, dtype=np.float32)).to(dev)
    status = torch.zeros((F,), dtype=torch.int32, device=dev)
    zmax = _hip.gt_paste_ground(batch.points6, batch.n_points, cfg.velorange, GRIDSHAPE)
    res = _hip.gt_paste_place(zmax, cfg.velorange, b2, b3, bv, n_host.to(dev), lim, cand_d, thr_d, db, status, iou_thr=BEV_IOU_THR,
                              debug=debug)
    picked, n_out = res[0], res[1]
    n_new = _hip.gt_paste_points(batch.points6, batch.n_points, picked, db, status)
    if images is not None:
        _hip.gt_paste_image(images, picked, db)
    S = picked.shape[1]
    geo, words = None, [picked.reshape(-1), n_out, n_new, status]
    if geometry is not None:
        from modules.augment import Geometry
        noise, glob, iou_thr = Geometry.geometry_draws(geometry, F, cap)
        geo = Geometry.launch(batch.points6, n_new, b3, n_out, noise, glob, iou_thr)
        words += geo.words()
    host = torch.cat(words).cpu().numpy()          # the one host read
    out = FramesResult()
    out.status = host[F * S + 2 * F:F * S + 3 * F].tolist()
    _raise_on(out.status)
    out.picked = [[int(p) for p in host[f * S:(f + 1) * S] if p >= 0] for f in range(F)]
    counts = host[F * S:F * S + F]
    out.n_points = host[F * S + F:F * S + 2 * F].tolist()
    out.boxes, out.bbox3d, out.bbox2d = [], [], []
    for f in range(F):
        k = int(counts[f])
        out.boxes.append((bv[f, :k], b3[f, :k, :2]) if k else None)
        out.bbox3d.append(b3[f, :k] if k else None)
        out.bbox2d.append(b2[f, :k] if k else None)
    out.debug = res[2:] if debug else None
    out.geometry = None
    batch.n_points = n_new
    if geo is not None:
        g = out.geometry = geo.finish(host[F * S + 3 * F:])
        out.boxes, out.bbox3d, out.bbox2d, out.n_points = g.boxes, g.bbox3d, None, g.n_points
        batch.points6, batch.n_points = geo.points6, geo.n_points
    if shuffle:
        perms = np.zeros(tuple(batch.perms.shape), np.int32)
        for f in range(F):
            a = np.arange(out.n_points[f], dtype=np.int32)
            np.random.shuffle(a)
            perms[f, :a.shape[0]] = a
        batch.perms = torch.from_numpy(perms).to(dev)
    return out
