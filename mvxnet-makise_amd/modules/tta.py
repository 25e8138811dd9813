"""Test-time augmentation for detection: V views of every frame through one forward, their detections fused (csrc/tta.hip).

A view is a row ``(phi, s, flip, 0)`` exactly as ``Geometry.draw_geometry`` writes ``glob``: a global rotation about z
(``Calc.getRotationMatrices`` on row vectors), a scale, then the y flip, then the range filter of ``cfg.velorange`` -- the
global step of ``geom_points``, which moves ``x y z`` only, so every point keeps the pixel it was seen at and the fusion layer
needs no second camera model.

  * ``views``: the rows from names or numbers;
  * ``expand_batch``: a FrameBatch of F * V frames, frame ``f * V + v`` = view v of source frame f, through the existing
    geometry launches (no new point kernel);
  * ``fuse_views``: the padded detections of the F * V frames -> one list per source frame, three launches: every box back
    into the source frame (the inverse of ``Geometry.transform_boxes``), greedy clusters in score order, score-weighted
    averages over at most one voter per view.

``detect.detect_frame_set(..., tta=views)`` puts the three together.  No claim about AP is made here: the mechanism is checked
against float64 (tests/tta_ref.py), its effect on a trained model is not measured.
"""
import math

import numpy as np
import torch

from modules import _hip
from modules import Extension as X

MAX_VIEWS = _hip.TTA_MAX_VIEWS
NAMES = ('identity', 'flip', 'rot+', 'rot-', 'flip+rot+', 'flip+rot-')


def views(spec, rot=math.pi / 8):
    """f32 (V, 4) view rows ``(phi, s, flip, 0)`` from ``spec``: a list whose items are rows (phi, s, flip[, 0]) or the names
    'identity', 'flip', 'rot+', 'rot-', 'flip+rot+', 'flip+rot-' (a single name or an array of rows is taken too).  A named
    rotation turns by ``+rot`` / ``-rot``; a named view has scale 1, other scales are given as rows.  The default ``rot`` of
    pi / 8 is a design choice (half of the training augmentation's pi / 4 range), not a measured optimum.  1..8 views."""
    if isinstance(spec, torch.Tensor):
        spec = spec.detach().cpu().numpy()
    if isinstance(spec, str):
        spec = [spec]
    if isinstance(spec, np.ndarray) and spec.ndim == 1:
        spec = [spec]
    rows = []
    for item in spec:
        if isinstance(item, str):
            if item not in NAMES:
                raise X.MvxHipError('unknown view %r: one of %s, or a row (phi, s, flip)' % (item, ', '.join(NAMES)))
            phi = float(rot) if 'rot+' in item else -float(rot) if 'rot-' in item else 0.0
            rows.append((phi, 1.0, 1.0 if 'flip' in item else 0.0, 0.0))
        else:
            r = [float(x) for x in np.asarray(item, dtype=np.float64).reshape(-1)]
            if len(r) not in (3, 4) or (len(r) == 4 and r[3] != 0.0):
                raise X.MvxHipError('a view row is (phi, s, flip) or (phi, s, flip, 0), not %r' % (item,))
            if not (math.isfinite(r[0]) and math.isfinite(r[1]) and r[1] > 0.0):
                raise X.MvxHipError('a view needs a finite angle and a positive scale, not %r' % (item,))
            rows.append((r[0], r[1], 1.0 if r[2] != 0.0 else 0.0, 0.0))
    if not 1 <= len(rows) <= MAX_VIEWS:
        raise X.MvxHipError('test-time augmentation takes 1..%d views, not %d' % (MAX_VIEWS, len(rows)))
    return np.asarray(rows, dtype=np.float32).reshape(-1, 4)


def options(args):
    """(keyword arguments of ``detect_frame_set`` for the parsed --tta / --tta-rot / --fuse-iou / --min-views switches of
    detect_like.py and visualize_like.py, number of views)."""
    if not args.tta:
        return {}, 1
    rows = views(args.tta, rot=args.tta_rot)
    return dict(tta=rows, fuse_iou=args.fuse_iou, min_views=args.min_views), rows.shape[0]


def _view_perm(f, v, n, cap):
    """The shuffle permutation of a view whose point count differs from its source's: seeded by (frame, view, count), so a run
    repeats."""
    row = np.zeros((cap,), np.int32)
    row[:n] = np.random.default_rng([f, v, n]).permutation(n).astype(np.int32)
    return row


def expand_batch(batch, view_rows):
    """A ``pipeline.FrameBatch`` of F * V frames from the F frames of ``batch``, view-major inside a source frame: frame
    ``f * V + v`` is view ``view_rows[v]`` of source frame f.  The prepared clouds (``batch.prepared()``: raw clouds are
    cropped and projected first) are replicated and sent through the global step and range filter of the geometric
    augmentation (``Geometry.launch`` with no boxes and zero noise); ``fpn_levels[f * V + v]`` is the source frame's list
    object, no feature map is copied; ``calib`` is carried along and ``raw`` dropped, the views being prepared clouds.  A view
    whose point count equals its source's keeps the source's shuffle permutation -- an identity row leaves points, count and
    order bitwise alone --, any other gets a seeded permutation over its new count.  ONE host read (the counts).  ``batch`` is
    not changed.  F * V above MVX_MAX_FRAMES raises."""
    from modules.augment import Geometry
    from modules.pipeline import FrameBatch
    view_rows = views(view_rows)
    F, V = batch.n_frames, view_rows.shape[0]
    if F * V > X.MAX_FRAMES:
        raise X.MvxHipError('%d frames x %d views = %d frames, a frame set holds at most %d' % (F, V, F * V, X.MAX_FRAMES))
    dev = batch.device
    pts, n_src = batch.prepared()
    if pts.dtype != torch.float32 or pts.dim() != 3 or pts.shape[2] != 6:
        raise X.MvxHipError('expand_batch needs clouds f32 (F, cap, 6), not %s' % (tuple(pts.shape),))
    cap = pts.shape[1]
    rep = pts.repeat_interleave(V, dim=0).contiguous()
    n_rep = n_src.to(torch.int32).repeat_interleave(V).contiguous()
    glob = np.tile(view_rows, (F, 1))
    run = Geometry.launch(rep, n_rep, torch.zeros((F * V, 1, 7), dtype=torch.float32, device=dev),
                          torch.zeros((F * V,), dtype=torch.int32, device=dev), np.zeros((F * V, 1, 1, 4), np.float32), glob)
    host = torch.cat([run.n_points, run.status, n_rep]).cpu().numpy()      # the one host read
    n_new, status, n_old = host[:F * V], host[F * V:2 * F * V], host[2 * F * V:]
    if status.any():
        raise X.MvxHipError('expand_batch: geometry status %s' % status.tolist())
    perms = None
    if batch.perms is not None:
        perms = batch.perms.repeat_interleave(V, dim=0).contiguous()
        changed = [k for k in range(F * V) if n_new[k] != n_old[k]]
        if changed:
            rows = np.stack([_view_perm(k // V, k % V, int(n_new[k]), perms.shape[1]) for k in changed])
            perms[torch.as_tensor(changed, device=dev)] = torch.from_numpy(rows).to(dev)
    fpn = [batch.fpn_levels[k // V] for k in range(F * V)]
    return FrameBatch(run.points6, perms, run.n_points, fpn, calib=batch.calib, cap_points=cap)


def fuse_views(dev_dets, view_rows, F, *, iou_thr, fuse_iou=0.5, min_views=1, out_max=None, full_turn=False, read=True):
    """One detection list per source frame from the V views' lists.  ``dev_dets``: the ``read=False`` dict of
    ``detect.postprocess`` over F * V frames (``boxes (F*V, post_max, 7)``, ``scores``, ``meta`` whose row 0 holds the counts),
    frame ``f * V + v`` being view v of source frame f; ``view_rows`` as ``views`` takes them (or its result, or that on the
    device).

    Every box goes back to the source frame; the union is scanned in score order (then view, then rank): an entry is a cluster
    head unless an earlier head overlaps it with BEV IoU > ``iou_thr`` -- the heads are the boxes a greedy NMS over the union
    keeps --, else it belongs to the first such head.  Per cluster at most one entry of each view votes, the first with
    IoU > ``fuse_iou`` to the head (the head votes for its own view); the fused box is the score-weighted mean of the voters
    (yaw differences wrapped into the half turn, or the full turn with ``full_turn`` -- a model with the direction head),
    the fused score the voters' score sum / V.  Clusters with fewer than ``min_views`` voters are dropped; at most ``out_max``
    (default ``post_max``) boxes per frame, fused score descending.  Averaging moves the heads: IoU <= iou_thr holds between the
    heads, not strictly between the fused boxes.  ``fuse_iou=0.5`` and ``min_views=1`` are design choices, not measured optima;
    for car-shaped boxes a fuse_iou above roughly 0.26 keeps voters a quarter turn off the head out.

    Returns F dicts ``{boxes (n,7), scores (n,), n_views (n,) i32, src (n,) i32 = view * post_max + rank of the head, status}``
    after ONE host read; ``read=False`` returns the device tensors ``{boxes (F,out_max,7), scores, n_views, src, meta i32 (2,F)
    = (counts, status)}``."""
    boxes, scores = dev_dets['boxes'], dev_dets['scores']
    dev = boxes.device
    if isinstance(view_rows, torch.Tensor) and view_rows.is_cuda:
        vdev = view_rows.detach().float().contiguous()
    else:
        vdev = torch.from_numpy(views(view_rows)).to(dev)
    V = vdev.shape[0]
    if boxes.shape[0] != F * V:
        raise X.MvxHipError('fuse_views: %d detection frames are not %d frames x %d views' % (boxes.shape[0], F, V))
    post_max = boxes.shape[1]
    out_max = post_max if out_max is None else int(out_max)
    if not (1e-3 <= iou_thr <= fuse_iou < 1.0) or not 1 <= min_views <= V or not 1 <= out_max <= V * post_max:
        raise X.MvxHipError('fuse_views: 1e-3 <= iou_thr <= fuse_iou < 1, 1 <= min_views <= V, 1 <= out_max <= V * post_max '
                            '(iou_thr %g, fuse_iou %g, min_views %d, V %d, out_max %d)' % (iou_thr, fuse_iou, min_views, V, out_max))
    counts = dev_dets['meta'][0].contiguous()
    res = _hip.tta_fuse_frames(boxes.contiguous(), scores.contiguous(), counts, vdev, F, iou_thr, fuse_iou, min_views, out_max,
                               full_turn)
    out = dict(boxes=res[0], scores=res[1], n_views=res[2], src=res[3], meta=res[4])
    return unpack(out) if read else out


def unpack(dev_out):
    """The device dict of ``fuse_views(read=False)`` -> per-frame dicts (one host read)."""
    counts, status = dev_out['meta'].tolist()
    return [dict(boxes=dev_out['boxes'][f, :n], scores=dev_out['scores'][f, :n], n_views=dev_out['n_views'][f, :n],
                 src=dev_out['src'][f, :n], status=status[f]) for f, n in enumerate(counts)]
