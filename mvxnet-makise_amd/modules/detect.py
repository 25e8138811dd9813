"""Detection output: the RPN's head output -> boxes per frame (csrc/detect.hip), and KITTI result files.

The reference stops at the score / regression maps (its Calc.decodeRegression is never called; no NMS, no eval).  Here:
  * ``postprocess``: score selection, top-K, box decoding and rotated BEV NMS of all frames of a step in four launches, one
    host read of the counts;
  * ``detect_frame_set``: the forward half of ``pipeline.train_step_full`` (frame sets through fusion / VFE / CML, the RPN on
    this library's kernels) followed by ``postprocess`` -- no parameter, gradient or gradient bucket is touched;
  * ``detect_frame_set(..., tta=views)``: test-time augmentation -- V views of every frame through the same forward, their
    lists fused per source frame (modules/tta.py, csrc/tta.hip);
  * ``boxes_lidar_to_camera`` / ``write_kitti_results``: KITTI ``label_2`` lines for the devkit.
"""
import math

import numpy as np
import torch

import modules.config as cfg
from modules import _hip
from modules import Extension as X

DEFAULTS = dict(score_thr=0.05, iou_thr=0.01, pre_max=1000, post_max=100, decode='loss')


def _anchors_dev(anchors, h1, w1, dev):
    """[h1][w1][A][7] f32 contiguous on ``dev`` (the (l, w, 7A) grid of Preprocessing.createAnchors is the same memory)."""
    from modules import Calc
    a = anchors if anchors.is_cuda else Calc._anchors_on(anchors, dev)
    a = a.detach().float().contiguous()
    return a.view(h1, w1, -1, 7)


def _views(heads_or_maps, F, h1, w1):
    """(cls (F,h1,w1,A), reg (F,h1,w1,7A), dir (F,h1,w1,A) or None, iou (F,h1,w1,A) or None) views of the channels-last heads
    (F*h1*w1, 16), of the direction model's (F*h1*w1, 20) = [cls | reg | dir | 0 0] (rpn_frames.head_layout), or of NCHW maps
    (cls, reg[, dir[, iou]]).  The last entry of a heads tensor is columns 9A..10A when the rows are that wide: whether they are
    IoU logits or padding the caller knows (``postprocess(iou=)``), the width does not tell."""
    if isinstance(heads_or_maps, (tuple, list)):
        cls, reg = heads_or_maps[:2]
        assert cls.dim() == 4 and cls.shape[0] == F and cls.shape[2:] == (h1, w1), tuple(cls.shape)
        assert reg.shape == (F, 7 * cls.shape[1], h1, w1), tuple(reg.shape)
        dirm = heads_or_maps[2] if len(heads_or_maps) > 2 else None
        assert dirm is None or dirm.shape == cls.shape, tuple(dirm.shape)
        ioum = heads_or_maps[3] if len(heads_or_maps) > 3 else None
        assert ioum is None or ioum.shape == cls.shape, tuple(ioum.shape)
        return (cls.permute(0, 2, 3, 1), reg.permute(0, 2, 3, 1), None if dirm is None else dirm.permute(0, 2, 3, 1),
                None if ioum is None else ioum.permute(0, 2, 3, 1))
    from modules import rpn_frames as rf
    v = heads_or_maps.view(F, h1, w1, -1)
    A, has_dir = rf.head_layout(v.shape[-1])
    return (v[..., :A], v[..., A:8 * A], v[..., 8 * A:9 * A] if has_dir else None,
            v[..., 9 * A:10 * A] if has_dir and v.shape[-1] >= 10 * A else None)


def postprocess(heads_or_maps, anchors, F, h1, w1, *, score_thr=0.05, iou_thr=0.01, pre_max=1000, post_max=100, decode='loss',
                read=True, debug=False, direction=None, dir_offset=math.pi / 4, iou=None, iou_alpha=0.5):
    """Boxes of F frames from the raw head output, read in place: the frame-set heads (F*h1*w1, 16) = [cls logits | reg] of
    ``rpn_frames.rpn_forward``, or NCHW maps ``(cls logits (F,2,h1,w1), reg (F,14,h1,w1))``.  ``anchors`` (h1, w1, 14) =
    [l][w][A][7] (Preprocessing.createAnchors), on the host or the device.

    Per frame: anchors with sigmoid(logit) >= score_thr, the best ``pre_max`` of them (logit descending, then anchor index
    ascending), decoded (``decode='loss'``: the inverse of VoxelLoss's targets; ``'reference'``: Calc.decodeRegression as the
    reference wrote it, diagonal from anchor columns 0:2), greedy NMS at BEV IoU > iou_thr, at most ``post_max`` kept.

    ``direction``: fold every decoded yaw into the half turn its direction logit names (the classifier that
    ``FocalLoss(direction=True)`` trains, with the same ``dir_offset``) and wrap it into [-pi, pi), before the corners and the
    NMS.  None (default) = when the heads carry direction columns (the 20-wide rows of a direction model, or a third map);
    True without them is an error, False ignores them.

    ``iou``: admit, rank and score the anchors by cls^(1-a) iou^a, a = ``iou_alpha`` in [0, 1], with the IoU logits of the head
    that ``FocalLoss(iou=True)`` trains -- columns 9A..10A of the rows of an IoU model
    (``MVXNet(direction=True, iou=True)``), or a fourth map.  With a heads tensor None means off: a 20-wide row does not tell
    whether its last two columns are IoU logits or the direction model's padding, so ``detect_frame_set`` / ``MVXNet.detect``
    pass ``hasattr(rpn, 'iou')``; with maps None means "a fourth map is there".  True without the columns is an error.
    ``iou_alpha = 0.5`` is a design choice taken over from those detectors' papers, not an optimum measured here; 0 is the plain score.

    Returns a list of F dicts ``{boxes (n,7) xyzlwhr, scores (n,), anchor_idx (n,) i32, n_candidates, status}`` (device
    tensors) after ONE device->host read; ``read=False`` returns the padded device tensors instead
    ``{boxes (F,post_max,7), scores, anchor_idx, meta i32 (3,F) = (counts, n_candidates, status)}`` for a caller that
    pipelines (``unpack`` reads them later).  ``debug`` adds the sorted candidates ('cand_idx', 'cand_boxes',
    'cand_corners', padded to pre_max) to the device dict."""
    cls, reg, dirv, iouv = _views(heads_or_maps, F, h1, w1)
    if iou is None:
        iou = iouv is not None and isinstance(heads_or_maps, (tuple, list))
    if iou and iouv is None:
        raise X.MvxHipError('postprocess(iou=True) needs heads with IoU columns (MVXNet(direction=True, iou=True)) or a fourth map')
    if iou and iouv.dtype != torch.float32:
        raise X.MvxHipError('postprocess reads f32 head outputs')
    if iou and not 0.0 <= float(iou_alpha) <= 1.0:
        raise X.MvxHipError('iou_alpha must lie in [0, 1], not %r' % (iou_alpha,))
    if direction is None:
        direction = dirv is not None
    if direction and dirv is None:
        raise X.MvxHipError('postprocess(direction=True) needs heads with direction columns (MVXNet(direction=True))')
    if direction and dirv.dtype != torch.float32:
        raise X.MvxHipError('postprocess reads f32 head outputs')
    if cls.dtype != torch.float32 or reg.dtype != torch.float32:
        raise X.MvxHipError('postprocess reads f32 head outputs')
    A = cls.shape[-1]
    anc = _anchors_dev(anchors, h1, w1, cls.device)
    if anc.shape[2] != A:
        raise X.MvxHipError('anchors hold %d orientations per cell, the heads %d' % (anc.shape[2], A))
    res = _hip.detect_frames(cls, reg, anc, F, h1, w1, A, score_thr, iou_thr, pre_max, post_max, decode, debug=debug,
                             dir_logits=dirv if direction else None, dir_offset=dir_offset, iou_logits=iouv if iou else None,
                             iou_alpha=iou_alpha)
    out = dict(boxes=res[0], scores=res[1], anchor_idx=res[2], meta=res[3])
    if debug:
        out.update(cand_idx=res[4], cand_boxes=res[5], cand_corners=res[6])
    return unpack(out) if read else out


def unpack(dev_out):
    """The device dict of ``postprocess(read=False)`` -> per-frame dicts (one host read)."""
    counts, n_cand, status = dev_out['meta'].tolist()
    return [dict(boxes=dev_out['boxes'][f, :n], scores=dev_out['scores'][f, :n], anchor_idx=dev_out['anchor_idx'][f, :n],
                 n_candidates=n_cand[f], status=status[f]) for f, n in enumerate(counts)]


def _empty(dev):
    return dict(boxes=torch.zeros((0, 7), device=dev), scores=torch.zeros((0,), device=dev),
                anchor_idx=torch.zeros((0,), dtype=torch.int32, device=dev), n_candidates=0, status=0)


def detect_frame_set(model, batch, anchors, imsize, ready=None, keep=None, tta=None, fuse_iou=0.5, min_views=1, **kw):
    """Detections for every frame of ``batch`` (pipeline.FrameBatch): the forward of ``pipeline.train_step_full`` -- the frame
    set through fusion / VFE / CML and the RPN on this library's kernels, per-frame BatchNorm statistics -- then
    ``postprocess`` (keyword arguments as there).  With ``bntrack`` it follows ``model.training``: a model in eval mode is
    normalised with its running statistics (modules/bn_running.py: one table launch in front of the first layer, no statistics
    pass where a layer has a form without), a model in training mode with the frames' own statistics as ever; the buffers are
    never written here.  ``ready``: a prepared frame set as train_step_full takes it (or None).
    Returns one dict per batch frame; frames without voxels get empty results.  Reads no gradient and writes none; the
    data-dependent status words are checked like ``pipeline.read_losses``.  ``keep`` (tests): receives 'heads', 'geom', the saved
    state of the forwards ('saved', 'rpn') and, with ``bntrack``, 'bn_sites'.

    ``tta`` (default None: nothing below happens, not a launch more): test-time augmentation, views as ``modules.tta.views``
    takes them.  The batch is expanded to F * V frames (``tta.expand_batch``; F * V <= 16), the same forward and ``postprocess``
    run over them and ``tta.fuse_views`` (``fuse_iou``, ``min_views`` as there; the full-turn yaw average when the model has the
    direction head) turns the views' lists into one per source frame.  The dicts keep 'boxes' / 'scores' and gain 'n_views' and
    'src'; 'anchor_idx' is the cluster head's, 'n_candidates' the sum and 'status' the OR over the frame's views (and the
    fusion's).  A source frame whose views are all empty gets the empty result.  ``ready`` cannot be combined with it."""
    if tta is not None:
        return _detect_tta(model, batch, anchors, imsize, ready, keep, tta, fuse_iou, min_views, kw)
    dets, live, _ = _detect_dev(model, batch, anchors, imsize, ready, keep, kw)
    out = [_empty(batch.device) for _ in range(batch.n_frames)]
    if dets is not None:
        for f, d in zip(live, unpack(dets)):
            out[f] = d
    return out


def _detect_dev(model, batch, anchors, imsize, ready, keep, kw, then=None):
    """The step of ``detect_frame_set`` up to the padded device tensors of ``postprocess(read=False)`` over the live frames:
    (that dict or None when no frame has a voxel, the live frames' ids, the result of ``then(dets, live)`` -- more launches
    inside the step's scope, on its arena -- or None).  The status words are checked here."""
    from modules import bn_running as bnr
    from modules import frames as fr
    from modules import pipeline as pl
    from modules import rpn_frames as rf
    opts = dict(DEFAULTS, **kw)
    opts.setdefault('iou', hasattr(model.backbone.rpn, 'iou'))
    dev = batch.device
    bn_step = bnr.step(model, train_entry=False)
    fs, live, counts, status = pl._take_ready(batch, ready, torch.cuda.current_stream(dev))
    hw = [float(imsize[0]), float(imsize[1])]
    statuses = [status]
    dets = extra = None
    with pl._step_scope(dev, train=False), bn_step as bn:
        if fs is not None:
            model.prepack()
            _hip.arena_begin(dev, doubles=1 << 22)
            F = len(live)
            with torch.no_grad():
                if bn is not None and bn.eval:
                    bn.fill(model, F)               # every site's (running_mean, 1/sqrt(running_var + eps)): one launch
                feat, saved = fr.rows_forward(model, fs, [batch.fpn_levels[f] for f in live], hw, statuses)
                fr.cml_forward(model, fs, feat, saved, statuses, want_bev=False)
                heads, rs = rf.rpn_forward(model.backbone.rpn, saved.x3, F, saved.D3, saved.H, saved.W, saved.C3)
                dets = postprocess(heads, anchors, F, rs['h1'], rs['w1'], read=False, **opts)
                if then is not None:
                    extra = then(dets, live)
            if keep is not None:
                keep.update(heads=heads, geom=(F, rs['h1'], rs['w1']), saved=saved, rpn=rs)
                if bn is not None:
                    keep['bn_sites'] = bn.records(F, fs.desc)
    pl._check_statuses(statuses)
    return dets, live, extra


def pad_frames(dets, live, n_frames):
    """The padded device dict of the live frames -> that of all ``n_frames`` frames, the others with count 0 and zero rows."""
    if len(live) == n_frames:
        return dets
    dev = dets['boxes'].device
    at = torch.as_tensor(list(live), dtype=torch.long, device=dev)
    out = {}
    for k, fill in (('boxes', 0), ('scores', 0), ('anchor_idx', -1)):
        t = torch.full((n_frames,) + tuple(dets[k].shape[1:]), fill, dtype=dets[k].dtype, device=dev)
        t[at] = dets[k]
        out[k] = t
    out['meta'] = torch.zeros((3, n_frames), dtype=torch.int32, device=dev)
    out['meta'][:, at] = dets['meta']
    return out


def _detect_tta(model, batch, anchors, imsize, ready, keep, views, fuse_iou, min_views, kw):
    from modules import tta
    if ready is not None:
        raise X.MvxHipError('detect_frame_set(tta=...) expands the batch itself: a prepared frame set (ready=) cannot go with it')
    rows = tta.views(views)
    F, V = batch.n_frames, rows.shape[0]
    dev = batch.device
    full_turn = getattr(model.backbone.rpn, 'dir', None) is not None and kw.get('direction') is not False

    def fuse(dets, live):                       # inside the step's scope: the workspace comes from its arena
        full = pad_frames(dets, live, F * V)
        return full, tta.fuse_views(full, rows, F, iou_thr=dict(DEFAULTS, **kw)['iou_thr'], fuse_iou=fuse_iou, min_views=min_views,
                                    full_turn=full_turn, read=False)
    dets, live, both = _detect_dev(model, tta.expand_batch(batch, rows), anchors, imsize, None, keep, kw, then=fuse)
    empty = dict(_empty(dev), n_views=torch.zeros((0,), dtype=torch.int32, device=dev),
                 src=torch.zeros((0,), dtype=torch.int32, device=dev))
    if dets is None:
        return [dict(empty) for _ in range(F)]
    full, fused = both
    heads_idx = torch.gather(full['anchor_idx'].view(F, -1), 1, fused['src'].clamp_min(0).long())
    host = torch.cat([fused['meta'].reshape(-1), full['meta'][1:].reshape(-1)]).tolist()      # the one host read
    counts, status = host[:F], host[F:2 * F]
    n_cand, st_views = host[2 * F:2 * F + F * V], host[2 * F + F * V:]
    out = []
    for f, n in enumerate(counts):              # n = 0 (every view empty): empty slices
        st = status[f]
        for v in range(V):
            st |= st_views[f * V + v]
        out.append(dict(boxes=fused['boxes'][f, :n], scores=fused['scores'][f, :n], anchor_idx=heads_idx[f, :n],
                        n_views=fused['n_views'][f, :n], src=fused['src'][f, :n], n_candidates=sum(n_cand[f * V:(f + 1) * V]),
                        status=st))
    return out


# ---- KITTI result files ----------------------------------------------------------------------------------------------
def _tensor(m):
    return m if isinstance(m, torch.Tensor) else torch.as_tensor(np.asarray(m))


def boxes_lidar_to_camera(boxes, calib):
    """(N,7) LiDAR-frame xyzlwhr -> camera-frame 'hwlxyzr' (KITTI label order): the exact inverse of ``Calc.bboxCam2Lidar``
    as ``Load.createDataset`` applies it.  Like the reference's loader this uses ``Tr_velo_to_cam`` only, WITHOUT
    ``R0_rect``: the written boxes are in the frame the training labels were read in, so a model's output goes back to the
    file it would have been trained from.  Float64 arithmetic on the host; returns a float64 tensor."""
    b = _tensor(boxes).detach().to('cpu', torch.float64).reshape(-1, 7)
    v2c = _tensor(calib['Tr_velo_to_cam']).to('cpu', torch.float64)
    xyz1 = torch.cat([b[:, :3], torch.ones((b.shape[0], 1), dtype=torch.float64)], 1)
    cam = torch.empty_like(b)
    cam[:, 0:3] = b[:, [5, 4, 3]]
    cam[:, 3:6] = (xyz1 @ v2c.T)[:, :3]
    cam[:, 6] = b[:, 6] + 0.5 * math.pi
    return cam


def kitti_lines(dets, calib, imsize):
    """KITTI ``label_2`` lines of one frame's detections (dict with 'boxes' (n,7) LiDAR xyzlwhr and 'scores' (n,)):
    ``Car -1 -1 alpha x1 y1 x2 y2 h w l x y z ry score`` with alpha = ry - atan2(x, z) and the 2-D box spanned by the eight
    corners (Calc.bbox3d2corner) taken to the camera frame like the box (Tr_velo_to_cam), projected through P2 and clipped
    to the image ``imsize`` = (height, width)."""
    from modules import Calc
    boxes = _tensor(dets['boxes']).detach().to('cpu', torch.float64).reshape(-1, 7)
    scores = _tensor(dets['scores']).detach().to('cpu', torch.float64).reshape(-1)
    if boxes.shape[0] == 0:
        return []
    cam = boxes_lidar_to_camera(boxes, calib)
    v2c = _tensor(calib['Tr_velo_to_cam']).to('cpu', torch.float64)
    p2 = _tensor(calib['P2']).to('cpu', torch.float64)
    corners = Calc.bbox3d2corner(boxes)                                           # (n, 8, 3) LiDAR frame
    hom = torch.cat([corners, torch.ones(corners.shape[:2] + (1,), dtype=torch.float64)], 2)
    uvw = hom @ (p2 @ v2c).T                                                      # (n, 8, 4)
    depth = uvw[..., 2].clamp_min(1e-6)
    u, v = uvw[..., 0] / depth, uvw[..., 1] / depth
    h_img, w_img = float(imsize[0]), float(imsize[1])
    x1 = u.min(1).values.clamp(0, w_img - 1)
    x2 = u.max(1).values.clamp(0, w_img - 1)
    y1 = v.min(1).values.clamp(0, h_img - 1)
    y2 = v.max(1).values.clamp(0, h_img - 1)
    lines = []
    for k in range(boxes.shape[0]):
        h, w, l, x, y, z, ry = cam[k].tolist()
        alpha = ry - math.atan2(x, z)
        lines.append('Car -1 -1 %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.4f'
                     % (alpha, x1[k], y1[k], x2[k], y2[k], h, w, l, x, y, z, ry, float(scores[k])))
    return lines


def write_kitti_results(path, dets, calib, imsize):
    """One frame's detections as a KITTI result file (``kitti_lines``); an empty file when there are none."""
    lines = kitti_lines(dets, calib, imsize)
    with open(path, 'w') as f:
        f.write(''.join(ln + '\n' for ln in lines))
