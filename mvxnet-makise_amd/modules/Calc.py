"""Box geometry and target assignment with the reference's names (modules/Calc.py).

``classifyAnchors`` -- the call train.py:46 makes per frame -- runs on the GPU (csrc/anchors.hip) and returns the
reference's ``(pi, ni, gi)`` with the same members in the same order; the box conversions are a few tensor
operations on a handful of boxes (label preparation) and stay plain torch, as in the reference.
"""
import math
import types
import weakref
from typing import Sequence, Tuple, Union

import numpy as np
import torch

from modules import _hip
from modules import Extension as X

index3d = Tuple[torch.Tensor, torch.Tensor, torch.Tensor]


def getRotationMatrices(r: torch.Tensor):
    c, s = torch.cos(r).reshape((-1, 1)), torch.sin(r).reshape((-1, 1))
    return torch.concat([c, -s, s, c], dim=1).reshape((-1, 2, 2))


def bbox3d2bev(bbox3ds: torch.Tensor) -> torch.Tensor:
    """(..., 7) xyzlwhr -> BEV corner points (..., 4, 2) (reference Calc.py:15-38: unit-square corners scaled by
    (l, w), multiplied from the right by the rotation matrix, shifted by (x, y))."""
    assert bbox3ds.shape[-1] >= 7
    lead = bbox3ds.shape[:-1]
    b = bbox3ds.reshape((-1, bbox3ds.shape[-1]))
    corners = torch.tensor([[0.5, 0.5], [-0.5, 0.5], [-0.5, -0.5], [0.5, -0.5]], dtype=b.dtype, device=b.device)
    res = corners[None] * b[:, None, [3, 4]]
    res = res @ getRotationMatrices(b[:, 6]) + b[:, None, [0, 1]]
    return res.reshape(lead + (4, 2)) if len(lead) > 0 else res[0]


def bbox3d2corner(bbox3ds: torch.Tensor) -> torch.Tensor:
    """(..., 7) -> the 8 corners (..., 8, 3): top face then bottom face (reference Calc.py:40-62)."""
    assert bbox3ds.shape[-1] >= 7
    lead = bbox3ds.shape[:-1]
    b = bbox3ds.reshape((-1, bbox3ds.shape[-1]))
    bev = bbox3d2bev(b)
    z = b[:, None, 2:3].expand(-1, 4, 1)
    h = b[:, None, 5:6].expand(-1, 4, 1)
    res = torch.concat([torch.concat([bev, z + h], dim=2), torch.concat([bev, z], dim=2)], dim=1)
    return res.reshape(lead + (8, 3)) if len(lead) > 0 else res[0]


def anchorCenterCells(gtCenters: torch.Tensor, anchors_shape, velorange: Sequence[float]):
    """Centre cell of every ground truth, the f32 arithmetic of reference Calc.py:91-94."""
    l = (velorange[3] - velorange[0]) / anchors_shape[0]
    w = (velorange[4] - velorange[1]) / anchors_shape[1]
    nls = ((gtCenters[:, 0] - velorange[0] - l / 2) / l + 0.5).long()
    nws = ((gtCenters[:, 1] - velorange[1] - w / 2) / w + 0.5).long()
    return nls, nws


def _window_radius(gts: torch.Tensor, anchors: torch.Tensor) -> int:
    """Cells around the centre that can reach IoU >= 0.1: the boxes must at least touch, i.e. the centres are closer
    than half the sum of the two diagonals (the centre cell itself may be half a cell off the box centre)."""
    def diag(q):
        return float(torch.linalg.norm(q[..., 0, :] - q[..., 2, :], dim=-1).max())
    cell = min(float((anchors[1, 0, 0] - anchors[0, 0, 0]).abs().max()) if anchors.shape[0] > 1 else math.inf,
               float((anchors[0, 1, 0] - anchors[0, 0, 0]).abs().max()) if anchors.shape[1] > 1 else math.inf)
    if not math.isfinite(cell) or cell <= 0:
        return 55
    return max(2, min(55, int(math.ceil((diag(gts) + diag(anchors[0, 0])) / 2 / cell)) + 2))


_CONSTANTS = {}             # name -> (key, weak reference to the tensor, value): ONE entry per name


def _constant(name, t, tag, make):
    """``make()`` for the tensor ``t``, a constant of the run (the anchor tables, train.py:59-60): kept while the same tensor
    object comes back."""
    key = (t.data_ptr(), tuple(t.shape), tag)
    hit = _CONSTANTS.get(name)
    if hit is None or hit[0] != key or hit[1]() is not t:
        hit = (key, weakref.ref(t), make())
        _CONSTANTS[name] = hit
    return hit[2]


def _anchors_on(anchors, dev, name='anchors'):
    """The device copy of the anchor grid; ``name`` 'anchors7': that of the (l,w,A,7) table of IgnoreRegions, kept beside it."""
    return _constant(name, anchors, str(dev), lambda: anchors.detach().float().contiguous().to(dev))


def _anchor_radius(anchors: torch.Tensor) -> int:
    """First window radius of assignAnchorsFrames from the anchor table alone (read once): the anchor's diagonal for both boxes,
    plus 2 cells, at most 55.  A larger box makes the kernel report status 1 and the call is replayed with twice the radius."""
    def make():
        corner = anchors[:2, :2].detach().float().cpu()
        return _window_radius(corner[0, 0], corner)
    return _constant('radius', anchors, str(anchors.device), make)


def _device_of(anchors, device):
    return torch.device(device) if device is not None else (anchors.device if anchors.is_cuda else X.device())


def replay_wider(radius, run):
    """``run(radius) -> (result, status word)`` until status bit 1 (a box reaches beyond the window) is clear or the radius is 55,
    with twice the radius each time.  Returns (result, status word, the radius that gave them)."""
    while True:
        res, st = run(radius)
        if not (st & 1 and radius < 55):
            return res, st, radius
        radius = min(55, 2 * radius)


def _frame_groups(out, live, boxes, radius_of, enqueue, decode, dev):
    """The one driver of target assignment: the frames ``live`` with their ``boxes`` ((n,4,2) each, n = 0 allowed) in groups of
    MAX_FRAMES.  Boxes that are device tensors stay on the device; host boxes are joined on the host and copied once;
    ``radius_of(the joined boxes)`` is the first window radius.
    ``enqueue(group, radius) -> (pos, neg, gi, words)`` launches a group -- ``group.ids`` its frames, ``group.gts`` their boxes back
    to back on the device, ``group.off`` the host offsets (F+1), ``group.first`` its first box among all -- and returns the raw
    device lists with ONE i32 device tensor, word 2F the status; it is read once per enqueue, and enqueued again through
    replay_wider (a widened radius stays for the groups that follow).  ``decode(host, group, status) -> counts`` (2F) gets the
    words as a list and raises what they report.  Fills and returns ``out``: out[frame] = ((x,y,z), (x,y,z), gi)."""
    boxes = [b.detach().float().reshape(-1, 4, 2) for b in boxes]
    joined = torch.cat([b.to(dev) for b in boxes] if any(b.is_cuda for b in boxes) else boxes).contiguous()
    radius, gts = radius_of(joined), joined.to(dev)
    off = [0]
    for b in boxes:
        off.append(off[-1] + b.shape[0])
    for lo in range(0, len(live), X.MAX_FRAMES):
        grp = types.SimpleNamespace(ids=live[lo:lo + X.MAX_FRAMES], first=off[lo])
        F = len(grp.ids)
        grp.off = [o - grp.first for o in off[lo:lo + F + 1]]
        grp.gts = gts[grp.first:grp.first + grp.off[-1]]

        def run(r):
            pos, neg, gi, words = enqueue(grp, r)
            host = words.tolist()                                            # the one host read of the group
            return (pos, neg, gi, host), host[2 * F]
        (pos, neg, gi, host), st, radius = replay_wider(radius, run)
        counts = decode(host, grp, st)
        for j, k in enumerate(grp.ids):
            n_pos, n_neg = counts[2 * j], counts[2 * j + 1]
            out[k] = ((pos[j, 0, :n_pos], pos[j, 1, :n_pos], pos[j, 2, :n_pos]),
                      (neg[j, 0, :n_neg], neg[j, 1, :n_neg], neg[j, 2, :n_neg]), gi[j, :n_pos])
    return out


def classifyAnchorsFrames(frames, anchors: torch.Tensor, velorange: Sequence[float], negThr: float, posThr: float, device=None):
    """classifyAnchors (train.py:46) for the frames of a step with ONE kernel pass and ONE host read: ``frames`` = per frame
    ``(gts (G,4,2), gtCenters (G,2))`` or None (no box).  Returns per frame ``(pi, ni, gi)`` exactly as classifyAnchors
    would (ground-truth ids local to the frame), or None."""
    dev = _device_of(anchors, device)
    live = [k for k, fr in enumerate(frames) if fr is not None and fr[0].shape[0] > 0]
    out = [None] * len(frames)
    if not live:
        return out
    a_dev = anchors if anchors.is_cuda else _anchors_on(anchors, dev)
    cen = torch.cat([frames[k][1].detach().float().cpu().reshape(-1, 2) for k in live])
    nls, nws = (t.to(dev) for t in anchorCenterCells(cen, anchors.shape, velorange))

    def enqueue(grp, r):
        sl = slice(grp.first, grp.first + grp.off[-1])
        pos, neg, gi, counts, status = _hip.classify_anchors_frames(grp.gts, grp.off, a_dev, nls[sl], nws[sl], negThr, posThr, r)
        return pos, neg, gi, torch.cat([counts.reshape(-1), status])

    def decode(host, grp, st):
        if st & 4:
            raise X.MvxHipError('classifyAnchors: a ground-truth centre lies outside the anchor grid '
                                '(the reference reads out of bounds there)')
        if st & 1:
            raise X.MvxHipError('classifyAnchors: a ground truth overlaps anchors more than 55 cells from its centre')
        return host[:2 * len(grp.ids)]

    def radius_of(gts):
        return _window_radius(gts.cpu(), anchors[:2, :2].detach().float().cpu())
    return _frame_groups(out, live, [frames[k][0] for k in live], radius_of, enqueue, decode, dev)


def classifyAnchors(gts: torch.Tensor, gtCenters: torch.Tensor, anchors: torch.Tensor, velorange: Sequence[float],
                    negThr: float, posThr: float, device=None) -> Tuple[index3d, index3d, torch.Tensor]:
    """Reference Calc.py:88-96 (-> cpp/voxelutil.cpp:138-316).  gts (G,4,2) BEV corners, gtCenters (G,2), anchors
    (L,W,A,4,2) BEV corners.  Returns ``(pi, ni, gi)``: index triples (LongTensors on the GPU) of the positive and of
    the not-negative anchors and the ground-truth id of every positive, in the reference's order.  One host read
    (the two list lengths and the status word).  classifyAnchorsFrames for one frame; three empty lists without a box."""
    res = classifyAnchorsFrames([(gts, gtCenters)], anchors, velorange, negThr, posThr, device)[0]
    return _empty_lists(_device_of(anchors, device)) if res is None else res


def _empty_lists(dev):
    e = torch.empty((0,), dtype=torch.int64, device=dev)
    return (e, e, e), (e, e, e), e


class IgnoreRegions:
    """The ignore sources of the frames of a step (csrc/ignore.hip), per frame and each optional (None or empty):
    ``rects`` (R,4) = (x1, y1, x2, y2) pixels -- DontCare rectangles -- with ``matrix`` (3,4) float64, LiDAR -> image;
    ``quads`` (B,4,2) BEV corners of look-alike boxes; ``boxes3d`` (G,7) the frame's Car boxes, whose points ``count_points``
    counts: a box with fewer than ``min_points`` (0 = off) is sparse.  ``anchors`` (l,w,A,7): the table whose BEV corners the
    assigner gets (needed by the rectangle rule: the anchor's centre).  ``ioa_thr``: intersection over the ANCHOR's area from which
    a look-alike box shields an anchor.  ``gt_points``: per frame i32 (G,) on the device or None, set by ``count_points``."""

    def __init__(self, n_frames, anchors=None, rects=None, matrix=None, quads=None, boxes3d=None, min_points=0, ioa_thr=0.5):
        def per_frame(v):
            v = [None] * n_frames if v is None else list(v)
            if len(v) != n_frames:
                raise ValueError('IgnoreRegions: %d entries for %d frames' % (len(v), n_frames))
            return v
        if not 0.0 < float(ioa_thr) <= 1.0:
            raise ValueError('IgnoreRegions: need 0 < ioa_thr <= 1, got %r' % (ioa_thr,))
        if int(min_points) < 0:
            raise ValueError('IgnoreRegions: need min_points >= 0, got %r' % (min_points,))
        self.n_frames, self.anchors = n_frames, anchors
        self.rects, self.matrix, self.quads, self.boxes3d = per_frame(rects), per_frame(matrix), per_frame(quads), per_frame(boxes3d)
        self.min_points, self.ioa_thr = int(min_points), float(ioa_thr)
        self.gt_points = [None] * n_frames
        for k in range(n_frames):
            if _rows(self.rects[k]) and self.matrix[k] is None:
                raise ValueError('IgnoreRegions: frame %d has rectangles and no matrix' % k)
        if any(_rows(r) for r in self.rects) and anchors is None:
            raise ValueError('IgnoreRegions: the rectangle rule needs the anchors (l,w,A,7)')

    def has_source(self, k):
        return bool(_rows(self.rects[k]) or _rows(self.quads[k]))

    def count_points(self, points6, n_points):
        """Counts the points of ``points6`` f32 (F, cap, ld) / ``n_points`` i32 (F,) (device) inside ``boxes3d``: one launch and
        one memset per MAX_FRAMES frames, no host read.  Nothing to do with ``min_points`` = 0."""
        self.gt_points = [None] * self.n_frames
        if self.min_points <= 0 or not any(_rows(b) for b in self.boxes3d):
            return self
        dev = points6.device
        for lo in range(0, self.n_frames, X.MAX_FRAMES):
            ids = list(range(lo, min(self.n_frames, lo + X.MAX_FRAMES)))
            sizes = [_rows(self.boxes3d[k]) for k in ids]
            if not any(sizes):
                continue
            off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
            b = torch.cat([torch.as_tensor(self.boxes3d[k]).detach().float()[:, :7].to(dev) for k in ids if _rows(self.boxes3d[k])])
            counts = _hip.box_point_counts_frames(points6[lo:lo + len(ids)], n_points[lo:lo + len(ids)], b.contiguous(),
                                                  torch.from_numpy(off).to(dev))
            for j, k in enumerate(ids):
                if sizes[j]:
                    self.gt_points[k] = counts[int(off[j]):int(off[j + 1])]
        return self


def _rows(t):
    return 0 if t is None else int(t.shape[0])


def _cat_rows(items, shape, dtype, dev):
    """Per-frame tensors / arrays / None -> (their rows back to back on ``dev`` or None when there is none, offsets i32 on ``dev``)."""
    sizes = [_rows(t) for t in items]
    if not any(sizes):
        return None, None
    parts = [torch.as_tensor(t).detach().to(dtype).reshape((-1,) + shape).to(dev) for t in items if _rows(t)]
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(dev)
    return torch.cat(parts).contiguous(), off


def _ignore_sources(ignore, grp, dev):
    """The sources of a group for _hip.ignore_anchors_frames, on the device: (gt_off, gt_points, rects, rect_off, mats, quads,
    quad_off), each None where the group has none."""
    ids = grp.ids
    rects, rect_off = _cat_rows([ignore.rects[k] for k in ids], (4,), torch.float32, dev)
    quads, quad_off = _cat_rows([ignore.quads[k] for k in ids], (4, 2), torch.float32, dev)
    mats = gt_points = gt_off = None
    if rects is not None:
        m = [np.zeros((3, 4)) if ignore.matrix[k] is None else np.asarray(ignore.matrix[k], np.float64).reshape(3, 4) for k in ids]
        mats = torch.from_numpy(np.stack(m)).to(dev)
    if ignore.min_points > 0 and any(ignore.gt_points[k] is not None for k in ids):
        parts = []
        for j, k in enumerate(ids):
            p, n = ignore.gt_points[k], grp.off[j + 1] - grp.off[j]
            if n and (p is None or p.shape[0] != n):
                raise ValueError('assignAnchors: frame %d holds %d boxes, its point counts are for %s'
                                 % (k, n, None if p is None else p.shape[0]))
            if n:
                parts.append(p.to(dev))
        gt_points = torch.cat(parts).contiguous()
        gt_off = torch.tensor(grp.off, dtype=torch.int32).to(dev)
    return gt_off, gt_points, rects, rect_off, mats, quads, quad_off


def assignAnchorsFrames(frames, anchors: torch.Tensor, negThr: float = 0.45, posThr: float = 0.6, forceThr: float = 0.1,
                        device=None, info=None, ignore=None):
    """Max-IoU assignment (csrc/assign.hip) for the frames of a step: an anchor is positive when its best IoU
    over the frame's boxes is >= posThr, or when it is the best anchor of a box whose best IoU is >= forceThr (forceThr > 1.5:
    thresholds only); not negative from negThr.  Every anchor at most once per list, in ascending (x, y, z) order.

    ``frames`` and the result are those of classifyAnchorsFrames: per frame ``(gts (G,4,2), gtCenters)`` or None in (the centres
    are not used: the kernel finds the centre cells, and a centre outside the grid is no error), ``(pi, ni, gi)`` or None out.
    Boxes that are device tensors stay on the device.  One host read per group of MAX_FRAMES frames (counts, status and the
    best IoU of every box together).  ``info`` (a dict) receives 'gt_best': per frame the best IoU of every box (CPU f32) or
    None, 'forced_only': the boxes whose best IoU lies in [forceThr, posThr) -- they owe their positive to the forced match --
    and 'none': the boxes below both (a box whose anchors all went to a box with an equal or better claim is not counted).

    ``ignore`` (default None: off, no ignore kernel and no ignore buffer): an IgnoreRegions for these frames.  The ignore pass
    (csrc/ignore.hip) then rewrites the raw device lists before the host read -- positives of sparse boxes are
    demoted, anchors over a DontCare rectangle or a look-alike box become not negative -- and its counts, status and stats ride
    in that same read; it is enqueued again on a radius replay.  A frame without boxes but with rectangles or look-alike boxes is
    live: it returns ``((e, e, e), ni, e)``.  ``info`` gains 'ignore_stats': [demoted positives, anchors newly ignored by a
    rectangle, newly ignored by a box only, sparse boxes], summed over the frames."""
    if not (0.0 < negThr <= posThr):
        raise ValueError('assignAnchors: need 0 < negThr <= posThr, got %r, %r' % (negThr, posThr))
    if not forceThr > 0.0:
        raise ValueError('assignAnchors: need forceThr > 0 (above 1.5 = no forced match), got %r' % (forceThr,))
    if ignore is not None and ignore.n_frames != len(frames):
        raise ValueError('assignAnchors: the IgnoreRegions hold %d frames, the call %d' % (ignore.n_frames, len(frames)))
    n_box = [0 if fr is None else int(fr[0].shape[0]) for fr in frames]
    live = [k for k in range(len(frames)) if n_box[k] > 0 or (ignore is not None and ignore.has_source(k))]
    out = [None] * len(frames)
    if info is not None:
        info.update(gt_best=[None] * len(frames), forced_only=0, none=0)
        if ignore is not None:
            info['ignore_stats'] = [0, 0, 0, 0]
    if not live:
        return out
    dev = _device_of(anchors, device)
    a_dev = anchors if anchors.is_cuda else _anchors_on(anchors, dev)
    if ignore is not None and ignore.anchors is not None:
        an7 = ignore.anchors.detach().float().contiguous() if ignore.anchors.is_cuda else _anchors_on(ignore.anchors, dev, 'anchors7')
        if an7.numel() != a_dev.numel() // 8 * 7:
            raise ValueError('assignAnchors: the IgnoreRegions hold another anchor table')
    elif ignore is not None:
        an7 = torch.zeros((a_dev.numel() // 8 * 7,), dtype=torch.float32, device=dev)       # never read: no rectangle
    sources = []                # [group, its sources on the device]: made once, a replay reuses them

    def enqueue(grp, r):
        if ignore is not None and (not sources or sources[0] is not grp):
            sources[:] = [grp, _ignore_sources(ignore, grp, dev)]
        pos, neg, gi, words = _hip.assign_anchors_frames(grp.gts, grp.off, a_dev, negThr, posThr, forceThr, r)
        if ignore is None:
            return pos, neg, gi, words
        gt_off, gt_points, rects, rect_off, mats, quads, quad_off = sources[1]
        pos, neg, gi, more = _hip.ignore_anchors_frames(pos, neg, gi, words[:2 * len(grp.ids)], an7, a_dev, gt_off, gt_points,
                                                        ignore.min_points, rects, rect_off, mats, quads, quad_off, ignore.ioa_thr)
        return pos, neg, gi, torch.cat([words, more])

    def decode(host, grp, st):
        """Words of the assigner: counts (2F), status, gt_best (G); of the ignore pass behind them: counts (2F), stats (4F), status."""
        if st & 1:
            raise X.MvxHipError('assignAnchors: a ground truth overlaps anchors more than 55 cells from its centre '
                                '(or the anchor table is no regular grid)')
        F, n_assign = len(grp.ids), 2 * len(grp.ids) + 1 + grp.off[-1]
        if ignore is not None and host[n_assign + 6 * F]:
            raise X.MvxHipError('assignAnchors: the ignore pass reports status %d' % host[n_assign + 6 * F])
        if info is not None:
            best = torch.tensor(host[2 * F + 1:n_assign], dtype=torch.int32).view(torch.float32)
            for j, k in enumerate(grp.ids):
                if ignore is not None:
                    stats = host[n_assign + 2 * F + 4 * j:n_assign + 2 * F + 4 * j + 4]
                    info['ignore_stats'] = [a + b for a, b in zip(info['ignore_stats'], stats)]
                if n_box[k]:
                    b = best[grp.off[j]:grp.off[j + 1]].clone()
                    forced = (b >= forceThr) & (b < posThr) if forceThr <= 1.5 else torch.zeros_like(b, dtype=torch.bool)
                    info['gt_best'][k] = b
                    info['forced_only'] += int(forced.sum())
                    info['none'] += int(((b < posThr) & ~forced).sum())
        return host[n_assign:n_assign + 2 * F] if ignore is not None else host[:2 * F]
    none = torch.zeros((0, 4, 2), dtype=torch.float32)
    return _frame_groups(out, live, [frames[k][0] if n_box[k] else none for k in live], lambda g: _anchor_radius(anchors), enqueue,
                         decode, dev)


def assignAnchors(gts: torch.Tensor, anchors: torch.Tensor, negThr: float = 0.45, posThr: float = 0.6, forceThr: float = 0.1,
                  device=None, info=None):
    """assignAnchorsFrames for one frame: ``(pi, ni, gi)``, three empty lists for a frame without boxes."""
    res = assignAnchorsFrames([(gts, None)], anchors, negThr, posThr, forceThr, device, info)[0]
    return _empty_lists(_device_of(anchors, device)) if res is None else res


def bboxCam2Lidar(camBoxes: Union[torch.Tensor, np.ndarray], c2v: Union[torch.Tensor, np.ndarray], inplace: bool = False):
    """(N,7) camera-frame 'hwlxyzr' -> lidar-frame 'xyzlwhr' (reference Calc.py:206-226)."""
    if not inplace:
        camBoxes = camBoxes.clone() if isinstance(camBoxes, torch.Tensor) else torch.as_tensor(np.array(camBoxes))
    xyz1 = torch.concat([camBoxes[:, 3:6], torch.ones((camBoxes.shape[0], 1))], dim=1).T
    xyz = (c2v @ xyz1).T
    camBoxes[:, 3:6] = camBoxes[:, [2, 1, 0]]
    camBoxes[:, :3] = xyz[:, :3]
    camBoxes[:, 6] = camBoxes[:, 6] - 0.5 * torch.pi
    return camBoxes


def decodeRegression(regmap: torch.Tensor, anchors: torch.Tensor) -> torch.Tensor:
    """Reference Calc.py:228-236, as written there (the diagonal is taken from columns 0:2)."""
    assert regmap.shape == anchors.shape
    d = torch.sqrt(anchors[..., [0]] ** 2 + anchors[..., [1]] ** 2)
    res = torch.empty(regmap.shape, device=regmap.device)
    res[..., :2] = regmap[..., :2] * d + anchors[..., :2]
    res[..., 2] = regmap[..., 2] * anchors[..., 5] + anchors[..., 2]
    res[..., 3:6] = torch.exp(regmap[..., 3:6]) * anchors[..., 3:6]
    res[..., 6] = regmap[..., 6] + anchors[..., 6]
    return res
