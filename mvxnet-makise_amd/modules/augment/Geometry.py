"""Geometric augmentation on the GPU (csrc/geom_augment.hip): per-object noise with a collision test, global scaling and
rotation (VoxelNet section 3.2) and the y flip of the common MVX-Net recipes, then the range filter.

The host draws every random number (``draw_geometry``; the draws do not depend on the outcomes) and the kernels do the rest:
``geom_place`` decides per box which of its trials is taken, moves the boxes and filters them, ``geom_points`` moves, filters
and compacts the points.  A frame's cloud is rows ``[x y z r row col]``: only ``x y z`` move, so every point keeps the image
position it was seen at -- the pairing the fusion layer samples, as an implementation that inverts the augmentation before
projecting gets it.

``augmentGeometryFrames`` is the frame-set form (three launches, one host read), ``augmentGeometry`` the single-frame case of
the same kernels; ``Augment.augmentFrames(..., geometry=...)`` runs the launches behind the GT paste inside its one read."""
import math

import numpy as np
import torch

import modules.config as cfg
from modules import _hip
from modules import Extension as X
from modules.augment.Augment import BEV_IOU_THR


class GeomParams:
    """Ranges of the draws.  VoxelNet section 3.2: ``rot_obj`` -- per-object rotation U[-pi/10, pi/10] about the box centre;
    ``sigma`` -- per-object shift N(0, 1) per axis; ``trials`` -- draws per object, the first without a collision is taken;
    ``scale`` -- global scaling U[0.95, 1.05]; ``rot_glob`` -- global rotation U[-pi/4, pi/4] about z.  ``flip_p``: probability
    of the y flip (MVX-Net recipes).  ``iou_thr``: two boxes collide above this BEV IoU -- the paste's threshold, so that
    "touching" means one thing in both."""
    __slots__ = ('rot_obj', 'sigma', 'trials', 'scale', 'rot_glob', 'flip_p', 'iou_thr')

    def __init__(self, rot_obj=math.pi / 10, sigma=(1.0, 1.0, 1.0), trials=16, scale=(0.95, 1.05), rot_glob=math.pi / 4, flip_p=0.5,
                 iou_thr=BEV_IOU_THR):
        if not 1 <= int(trials) <= _hip.GEOM_MAX_TRIALS:
            raise X.MvxHipError('trials is 1..%d' % _hip.GEOM_MAX_TRIALS)
        if not (0.0 < scale[0] <= scale[1]) or rot_obj < 0 or rot_glob < 0 or not 0.0 <= flip_p <= 1.0 or min(sigma) < 0:
            raise X.MvxHipError('GeomParams: a range is empty or negative')
        self.rot_obj, self.sigma, self.trials = float(rot_obj), tuple(float(s) for s in sigma), int(trials)
        self.scale, self.rot_glob, self.flip_p, self.iou_thr = (float(scale[0]), float(scale[1])), float(rot_glob), float(flip_p), float(iou_thr)


def draw_geometry(F, B, params, rng):
    """(noise f32 (F, B, T, 4) = (dx, dy, dz, dtheta), glob f32 (F, 4) = (phi, s, flip, 0)) from the ``np.random.Generator``
    ``rng``: always F * B * T * 4 + 3 F numbers in one order, whatever the frames hold."""
    T = params.trials
    noise = np.empty((F, B, T, 4), np.float32)
    noise[..., :3] = rng.normal(0.0, 1.0, (F, B, T, 3)) * np.asarray(params.sigma)
    noise[..., 3] = rng.uniform(-params.rot_obj, params.rot_obj, (F, B, T))
    glob = np.zeros((F, 4), np.float32)
    glob[:, 0] = rng.uniform(-params.rot_glob, params.rot_glob, F)
    glob[:, 1] = rng.uniform(params.scale[0], params.scale[1], F)
    glob[:, 2] = rng.random(F) < params.flip_p
    return noise, glob


def geometry_draws(geometry, F, B):
    """``geometry`` as the callers pass it -- a GeomParams, or a dict with 'params' (GeomParams), 'rng' (np.random.Generator)
    and optionally the draws themselves, 'noise' / 'glob' -> (noise, glob, iou_thr)."""
    if isinstance(geometry, GeomParams):
        geometry = {'params': geometry}
    params = geometry.get('params') or GeomParams()
    noise, glob = geometry.get('noise'), geometry.get('glob')
    if noise is None or glob is None:
        rng = geometry.get('rng')
        if rng is None:
            rng = geometry['rng'] = np.random.default_rng()
        noise, glob = draw_geometry(F, B, params, rng)
    return noise, glob, geometry.get('iou_thr', params.iou_thr)


def global_matrix(glob_row):
    """The global step of a frame as a 4x4 float64 matrix G on column vectors (x, y, z, 1): ``glob_row`` = (phi, s, flip, 0) as
    drawn (f32).  Exactly what geom_points / geom_place apply: p_xy <- s (p_xy @ R(phi)) with R of Calc.getRotationMatrices on row
    vectors, p_z <- s p_z, then y <- -y with the flip.  Points keep the pixel they were seen at, so a LiDAR -> image matrix M of
    the frame before the augmentation becomes M @ inv(G) behind it."""
    g = np.asarray(glob_row, np.float32).astype(np.float64)
    c, s, k = math.cos(g[0]), math.sin(g[0]), g[1]
    sy = -1.0 if g[2] != 0.0 else 1.0
    m = np.eye(4)
    m[0, :2] = [k * c, k * s]
    m[1, :2] = [-sy * k * s, sy * k * c]
    m[2, 2] = k
    return m


def transform_boxes(boxes7, glob_row):
    """Boxes (n, 7) xyzlwhr through the global step of ``glob_row``, as geom_place moves the frame's own boxes (without its
    per-object noise and range filter): the centre through ``global_matrix``, the sizes scaled, the yaw + phi, negated by the
    flip, wrapped into [-pi, pi).  Returns f32 (n, 7) of the input's kind (numpy or host tensor)."""
    is_t = isinstance(boxes7, torch.Tensor)
    b = (boxes7.detach().cpu().numpy() if is_t else np.asarray(boxes7)).astype(np.float32).astype(np.float64).reshape(-1, 7)
    g = np.asarray(glob_row, np.float32).astype(np.float64)
    G = global_matrix(glob_row)
    out = np.empty_like(b)
    out[:, :3] = (np.concatenate([b[:, :3], np.ones((b.shape[0], 1))], axis=1) @ G.T)[:, :3]
    out[:, 3:6] = g[1] * b[:, 3:6]
    r = b[:, 6] + g[0]
    if g[2] != 0.0:
        r = -r
    out[:, 6] = r - 2.0 * math.pi * np.floor((r + math.pi) / (2.0 * math.pi))
    out = out.astype(np.float32)
    return torch.from_numpy(out) if is_t else out


class GeomLaunched:
    """The enqueued launches of a frame set: device outputs, and the int32 words the host needs (``words``) so that a caller
    with a read of its own can carry them in it; ``finish`` turns the words into the per-frame result."""
    __slots__ = ('placed', 'points6', 'n_points', 'status', 'F', 'B')

    def words(self):
        return [self.placed.trial.reshape(-1), self.placed.kept_idx.reshape(-1), self.placed.n_kept, self.n_points, self.status]

    def n_words(self):
        return 2 * self.F * self.B + 3 * self.F

    def finish(self, host):
        """``host``: the words as a host int array -> GeomResult."""
        F, B = self.F, self.B
        host = np.asarray(host)
        out = GeomResult()
        out.trials = host[:F * B].reshape(F, B)
        out.kept = [[int(i) for i in row if i >= 0] for row in host[F * B:2 * F * B].reshape(F, B)]
        counts = host[2 * F * B:2 * F * B + F]
        out.n_points = host[2 * F * B + F:2 * F * B + 2 * F].tolist()
        out.status = host[2 * F * B + 2 * F:2 * F * B + 3 * F].tolist()
        if any(out.status):
            raise X.MvxHipError('geometric augmentation: status %s (2 = box count outside the table)' % out.status)
        p = self.placed
        out.boxes, out.bbox3d = [], []
        for f in range(F):
            k = int(counts[f])
            out.boxes.append((p.bev[f, :k], p.box3d[f, :k, :2]) if k else None)
            out.bbox3d.append(p.box3d[f, :k] if k else None)
        out.bbox2d = None
        out.moves = p.move
        return out


class GeomResult:
    """``boxes`` per frame ``(bev (n,4,2), centres (n,2))`` or None and ``bbox3d`` per frame (n,7) or None, on the device, as
    Calc.classifyAnchorsFrames and Augment.FramesResult hold them; ``bbox2d`` None (the 2-D boxes are stale); ``trials`` i32
    (F, B) the taken trial per input box (-1 none); ``moves`` f32 (F, B, 4) on the device; ``kept`` per frame the input
    indices of the boxes that stayed; ``n_points`` the new counts; ``status`` per frame."""
    __slots__ = ('boxes', 'bbox3d', 'bbox2d', 'trials', 'moves', 'kept', 'n_points', 'status')


def box_table(bbox3ds, dev, cap=None):
    """Per-frame (n, 7) boxes or None -> (f32 (F, cap, 7) on ``dev``, counts i32 (F,) on ``dev``)."""
    cap = _hip.GT_PASTE_MAX_BOXES if cap is None else cap
    F = len(bbox3ds)
    t = torch.zeros((F, cap, 7))
    n = torch.zeros((F,), dtype=torch.int32)
    for f, b in enumerate(bbox3ds):
        if b is None or b.shape[0] == 0:
            continue
        if b.shape[0] > cap:
            raise X.MvxHipError('a frame holds %d boxes, the placement takes at most %d' % (b.shape[0], cap))
        t[f, :b.shape[0]] = torch.as_tensor(b).detach().float().cpu()[:, :7]
        n[f] = b.shape[0]
    return t.to(dev), n.to(dev)


def launch(points6, n_points, box3d, n_box, noise, glob, iou_thr=BEV_IOU_THR, status=None, velorange=None):
    """Enqueues the launches for a frame set: box3d f32 (F, B, 7) / n_box i32 (F,) on the device, noise / glob numpy or
    device tensors.  No host read."""
    dev = points6.device
    F, B = box3d.shape[0], box3d.shape[1]
    velorange = cfg.velorange if velorange is None else velorange
    as_dev = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    noise, glob = as_dev(noise), as_dev(glob)
    if noise.shape[:2] != (F, B) or glob.shape != (F, 4):
        raise X.MvxHipError('noise is (F, B, T, 4) and glob (F, 4) for F = %d frames and B = %d box slots' % (F, B))
    out = GeomLaunched()
    out.F, out.B = F, B
    out.status = torch.zeros((F,), dtype=torch.int32, device=dev) if status is None else status
    out.placed = _hip.geom_place(box3d, n_box, noise, glob, velorange, out.status, iou_thr=iou_thr)
    out.points6, out.n_points = _hip.geom_points(points6, n_points, box3d, n_box, out.placed, glob, velorange)
    return out


def draw_perms(batch, n_points):
    """The shuffle permutations over the new counts, as augmentFrames draws them (the permutation stays an input of the voxelizer)."""
    perms = np.zeros(tuple(batch.perms.shape), np.int32)
    for f, k in enumerate(n_points):
        a = np.arange(k, dtype=np.int32)
        np.random.shuffle(a)
        perms[f, :k] = a
    batch.perms = torch.from_numpy(perms).to(batch.device)


def augmentGeometryFrames(batch, boxes, noise=None, glob=None, params=None, rng=None, iou_thr=None, shuffle=True):
    """The geometric augmentation for the frames of ``batch`` (pipeline.FrameBatch with prepared ``points6`` / ``n_points``).
    ``boxes``: per frame the 3-D boxes (n, 7) or None.  ``noise`` (F, 32, T, 4) / ``glob`` (F, 4): the draws, made here from
    ``rng`` by ``params`` when None.  ``batch.points6`` / ``batch.n_points`` are replaced and -- after the ONE host read of the
    call (trials, kept boxes, counts, status) -- the shuffle permutations are drawn over the new counts into ``batch.perms``
    (``shuffle``).  Returns a GeomResult."""
    dev = batch.device
    F = batch.n_frames
    b3, n_box = box_table(boxes, dev)
    if noise is None or glob is None:
        noise, glob, thr = geometry_draws({'params': params, 'rng': rng}, F, b3.shape[1])
        iou_thr = thr if iou_thr is None else iou_thr
    if iou_thr is None:
        iou_thr = (params or GeomParams()).iou_thr
    run = launch(batch.points6, batch.n_points, b3, n_box, noise, glob, iou_thr)
    out = run.finish(torch.cat(run.words()).cpu().numpy())          # the one host read
    batch.points6, batch.n_points = run.points6, run.n_points
    if shuffle:
        draw_perms(batch, out.n_points)
    return out


def augmentGeometry(pcd6, bbox3d, noise=None, glob=None, params=None, rng=None, iou_thr=None):
    """One frame: ``pcd6`` (P, 6) rows [x y z r row col] (numpy), ``bbox3d`` (n, 7) or None.  ``noise`` (32, T, 4) / ``glob``
    (4,), or drawn from ``rng`` by ``params``.  Returns (the new cloud (P', 6) f32 numpy, the new boxes (n', 7) and their bev
    (n', 4, 2) as host tensors, or None, None when no box is left)."""
    from modules.pipeline import FrameBatch
    dev = X.device()
    p = np.ascontiguousarray(pcd6, dtype=np.float32)
    P = p.shape[0]
    pts = torch.zeros((1, max(1, P), 6), dtype=torch.float32, device=dev)
    pts[0, :P] = torch.from_numpy(p).to(dev)
    batch = FrameBatch(pts, None, torch.tensor([P], dtype=torch.int32, device=dev), [None])
    if noise is not None and glob is not None:
        noise, glob = np.asarray(noise, np.float32)[None], np.asarray(glob, np.float32)[None]
    res = augmentGeometryFrames(batch, [bbox3d], noise, glob, params, rng, iou_thr, shuffle=False)
    cloud = batch.points6[0, :res.n_points[0]].cpu().numpy()
    if res.bbox3d[0] is None:
        return cloud, None, None
    return cloud, res.bbox3d[0].cpu(), res.boxes[0][0].cpu()
