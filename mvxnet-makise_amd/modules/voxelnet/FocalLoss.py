"""Focal loss for the RPN heads (Lin et al., "Focal Loss for Dense Object Detection"; the classification loss of SECOND,
PointPillars and mmdetection3d's MVXNet), for all frames of a step in one HIP call (csrc/loss_frames.hip):

    positive = listed in pi;  ignored = listed in ni (classifyAnchors' NOT-negative anchors) and not positive;  negative = the rest
    clsLoss = cls_weight / max(1, len(pi)) * ( sum_positive alpha (1-p)^gamma (-log p) + sum_negative (1-alpha) p^gamma (-log(1-p)) )
    regLoss = reg_weight * VoxelLoss's regLoss               (same targets, SmoothL1, mean over len(pi) * 7)

with p = sigmoid(logit).  It reads the raw head output -- logits, not probabilities: a focal loss from probabilities that
have saturated to 0 or 1 in f32 cannot be computed -- so it is used through ``heads_loss_frames`` on the frame-set path
(``pipeline.train_step_full(..., criterion=FocalLoss())``) and not through the reference's per-frame ``forward``.

``direction=True`` trains the heading the way those three detectors do, on a model built with
``MVXNet(direction=True)``.  Per ``pi`` entry, with D = reg[6] - (gt[6] - anchor[6]) and x the anchor's direction logit:

    the angle column of regLoss is SmoothL1(sin D) in place of SmoothL1(D): blind to half turns of the box
    b       = floor(mod(gt[6] - dir_offset, 2 pi) / pi)                       the half turn that is meant, 0 or 1
    dirLoss = dir_weight / max(1, len(pi)) * sum (b ? -log sigmoid(x) : -log(1 - sigmoid(x)))

and the decode (modules/detect.py) folds the regressed yaw into the half turn the logit names.  ``dir_weight=0.2`` and
``dir_offset=pi/4`` are the values of SECOND's and mmdetection3d's KITTI configurations: design choices taken over from
there, not optima measured on this model.

``iou=True`` (with ``direction=True``) trains the IoU-aware confidence head of CIA-SSD / AFDetV2 on a model
built with ``MVXNet(direction=True, iou=True)``.  Per ``pi`` entry, with x the anchor's IoU logit and the anchor's regression
row read as a constant (nothing flows into the regression from this term):

    q       = 3D IoU of the box the regression currently decodes (modules/detect.py, decode='loss') with its ground truth
    iouLoss = iou_weight / max(1, len(pi)) * sum (-q log sigmoid(x) - (1 - q) log(1 - sigmoid(x)))

and the decode ranks and scores by sigmoid(cls)^(1-a) sigmoid(x)^a.  ``iou_weight=1.0`` (and the decode's ``iou_alpha=0.5``)
are design choices in the range those papers use, not optima measured on this model.

``iou_loss=True`` (with every combination of ``direction`` and ``iou``) adds the rotated 3D IoU regression loss of
Zhou et al. (3DV 2019; SE-SSD's ODIoU, mmdetection3d's RotatedIoU3DLoss) to regLoss, with its analytic gradient flowing into the
seven regression columns.  Per ``pi`` entry, with q as above but differentiated:

    regLoss += iou_loss_weight / max(1, len(pi)) * sum (1 - q)

SmoothL1 stays in the sum: ``1 - q`` alone has no gradient for a positive that does not overlap its box, and forced positives
start at an IoU of 0.1.  ``iou_loss_weight=1.0`` is a design choice, not an optimum measured on this model.
"""
import collections
import math

import numpy as np
import torch
from torch import nn

from modules import _hip
from modules import Extension as X

PackedTargets = collections.namedtuple('PackedTargets', 'pos_idx neg_idx gi counts gts gt_off')


def _length(col):
    return int(col.shape[0]) if hasattr(col, 'shape') else len(col)


def _on_device(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


class FocalLoss(nn.Module):

    def __init__(self, alpha=0.25, gamma=2.0, cls_weight=1.0, reg_weight=2.0, direction=False, dir_weight=0.2, dir_offset=math.pi / 4,
                 iou=False, iou_weight=1.0, iou_loss=False, iou_loss_weight=1.0):
        super().__init__()
        if iou and not direction:
            raise X.MvxHipError('FocalLoss(iou=True) needs direction=True: the IoU logits take the two pad columns of the direction '
                                'model\'s head rows')
        self.alpha, self.gamma, self.cls_weight, self.reg_weight = alpha, gamma, cls_weight, reg_weight
        self.direction, self.dir_weight, self.dir_offset = bool(direction), dir_weight, dir_offset
        self.iou, self.iou_weight = bool(iou), iou_weight
        if not iou_loss_weight >= 0:
            raise X.MvxHipError('FocalLoss(iou_loss_weight=%r) must not be negative' % (iou_loss_weight,))
        self.iou_loss, self.iou_loss_weight = bool(iou_loss), iou_loss_weight
        self.last_box_iou = None           # (F,2) on the device = (the IoU term, mean IoU of the positives) of the last call

    def forward(self, pi, ni, gi, gts, score, reg, anchors, anchorsPerLoc):
        raise NotImplementedError('FocalLoss needs the logits of the heads, not their probabilities (a focal loss from '
                                  'probabilities saturated in f32 is not computable): call heads_loss_frames, or pass the '
                                  'criterion to pipeline.train_step_full')

    @staticmethod
    def pack_targets(targets, dev):
        """Per-frame ``(pi, ni, gi, gts)`` or None, as pipeline.train_step_full receives them -> (PackedTargets on ``dev``,
        has_reg): pos_idx / neg_idx i64 (F,3,cap), gi i64 (F,cap), counts i32 (F,2), gts f32 (max(1,n),7) of all frames
        back to back, gt_off i32 (F+1,); has_reg = per frame "has a positive".  The three index tensors are slices of ONE
        buffer, counts and gt_off of another.  Host lists reach the device with one copy per buffer; lists that are already
        there (Calc.classifyAnchorsFrames) are gathered by one concatenation and one indexed write -- in both cases the number
        of copies and launches does not depend on F."""
        F = len(targets)
        live = [t if t is not None else ((), (), (), None) for t in targets]
        pis = [t[0] if t[0] is not None and len(t[0]) == 3 else None for t in live]
        nis = [t[1] if t[1] is not None and len(t[1]) == 3 else None for t in live]
        n_pos = [0 if p is None else _length(p[0]) for p in pis]
        n_neg = [0 if n is None else _length(n[0]) for n in nis]
        cap = max(1, max(n_pos + n_neg))
        boxes = [t[3] for t in live]
        meta = np.zeros((3 * F + 1,), np.int32)                    # counts (F,2) | gt_off (F+1,)
        meta[0:2 * F:2], meta[1:2 * F:2] = n_pos, n_neg
        meta[2 * F + 1:] = np.cumsum([0 if b is None else int(b.shape[0]) for b in boxes])
        # one i64 buffer [pos (F,3,cap) | neg (F,3,cap) | gi (F,cap)]; its filled columns as (column, offset) pairs
        neg0, gi0 = 3 * F * cap, 6 * F * cap
        cols = []
        for f in range(F):
            if n_pos[f]:
                cols += [(c, (f * 3 + j) * cap) for j, c in enumerate(pis[f])] + [(live[f][2], gi0 + f * cap)]
            if n_neg[f]:
                cols += [(c, neg0 + (f * 3 + j) * cap) for j, c in enumerate(nis[f])]
        if not any(_on_device(c) for c, _ in cols):
            host = np.zeros((7 * F * cap,), np.int64)
            for c, off in cols:
                a = np.asarray(c, dtype=np.int64).reshape(-1)
                host[off:off + a.shape[0]] = a
            idx = torch.from_numpy(host).to(dev)
        else:
            idx = torch.empty((7 * F * cap,), dtype=torch.int64, device=dev)          # beyond the counts: never read
            dst = torch.from_numpy(np.concatenate([np.arange(off, off + _length(c), dtype=np.int64) for c, off in cols])).to(dev)
            idx[dst] = torch.cat([torch.as_tensor(c).to(dev, torch.int64).reshape(-1) for c, _ in cols])
        rows = [b.detach()[:, :7].float() for b in boxes if b is not None]
        if not rows:
            gts = torch.zeros((1, 7), dtype=torch.float32, device=dev)
        elif any(_on_device(b) for b in rows):
            gts = torch.cat([b.to(dev) for b in rows]).contiguous()
        else:
            gts = torch.cat(rows).contiguous().to(dev)
        meta = torch.from_numpy(meta).to(dev)
        packed = PackedTargets(idx[:neg0].view(F, 3, cap), idx[neg0:gi0].view(F, 3, cap), idx[gi0:].view(F, cap),
                               meta[:2 * F].view(F, 2), gts, meta[2 * F:])
        return packed, [n > 0 for n in n_pos]

    def heads_loss_frames(self, heads, F, h1, w1, targets, anchors, want_grads=True):
        """The loss of every frame on the channels-last head output (F*h1*w1, 8A) = [cls logits | reg] and its gradient, in
        one library call.  Returns (losses (F,2) on the device = (clsLoss, regLoss or 0), per-frame bool "has a regression
        loss", d_heads) -- the triple of pipeline.heads_loss.  With ``direction`` the rows are those of a direction model,
        [cls | reg | dir logits | zeros] (rpn_frames.head_layout), losses is (F,3) = (clsLoss, regLoss or 0, dirLoss) and
        d_heads carries the direction gradient in its columns, zeros in the pad columns.  A criterion and rows that do not
        match raise MvxHipError before anything is launched.  With ``iou`` the rows are those of an IoU model, [cls | reg | dir
        logits | iou logits] (columns 9A..10A), losses is (F,4) = (clsLoss, regLoss or 0, dirLoss, iouLoss) and d_heads carries
        the IoU gradient in those columns.  With ``iou_loss`` the regression loss (column 1) includes the rotated IoU term and
        d_heads its gradient in the regression columns; the widths and meanings are otherwise unchanged, and ``last_box_iou``
        keeps the (F,2) device tensor (term, mean IoU of the frame's positives) of this call (no host read)."""
        from modules import rpn_frames as rf
        if not heads.is_cuda:
            raise X.MvxHipError('FocalLoss runs on the GPU (no CPU fallback)')
        dev = heads.device
        A, has_dir = rf.head_layout(heads.shape[1])
        if has_dir != self.direction:
            raise X.MvxHipError('FocalLoss(direction=True) needs the heads of a direction model (MVXNet(direction=True)), and a '
                                'direction model needs FocalLoss(direction=True): the criterion has direction=%s, the heads are '
                                '%d wide' % (self.direction, heads.shape[1]))
        packed, has_reg = self.pack_targets(targets, dev)
        anc = anchors.detach().float().contiguous()
        if not anc.is_cuda:
            from modules import Calc
            anc = Calc._anchors_on(anchors, dev)
        if self.iou:
            if heads.shape[1] < 10 * A:
                raise X.MvxHipError('FocalLoss(iou=True) reads the IoU logits from columns %d..%d of the head rows; these are %d '
                                    'wide' % (9 * A, 10 * A, heads.shape[1]))
            losses, d_heads = _hip.focal_loss_iou_frames(heads, heads[:, 8 * A:9 * A], heads[:, 9 * A:10 * A], F, h1, w1, A,
                                                         packed.pos_idx, packed.neg_idx, packed.gi, packed.counts, packed.gts,
                                                         packed.gt_off, anc, self.alpha, self.gamma, self.cls_weight, self.reg_weight,
                                                         self.dir_weight, self.dir_offset, self.iou_weight, want_grads=want_grads)[:2]
        elif self.direction:
            losses, d_heads, _ = _hip.focal_loss_dir_frames(heads, heads[:, 8 * A:9 * A], F, h1, w1, A, packed.pos_idx, packed.neg_idx,
                                                            packed.gi, packed.counts, packed.gts, packed.gt_off, anc, self.alpha,
                                                            self.gamma, self.cls_weight, self.reg_weight, self.dir_weight,
                                                            self.dir_offset, want_grads=want_grads)
        else:
            losses, d_heads = _hip.focal_loss_frames(heads, F, h1, w1, A, packed.pos_idx, packed.neg_idx, packed.gi, packed.counts,
                                                     packed.gts, packed.gt_off, anc, self.alpha, self.gamma, self.cls_weight,
                                                     self.reg_weight, want_grads=want_grads)
        if self.iou_loss:
            # behind the focal call, on the d_heads it has just written: the term goes into column 1 of the losses on the device
            self.last_box_iou = _hip.box_iou_loss_frames(heads, F, h1, w1, A, packed.pos_idx, packed.gi, packed.counts, packed.gts,
                                                         packed.gt_off, anc, self.iou_loss_weight, want_grads=want_grads,
                                                         d_heads=d_heads, loss_add=losses[:, 1:2])[0]
        return losses, has_reg, d_heads
