"""Float64 restatement of the focal loss's contract (include/mvx_hip.h "Focal loss of the RPN heads") in
plain torch on the CPU, from the logits; it imports nothing of the package.  Membership is by SET (an anchor listed twice
counts once), the regression term is taken once per pos_idx ENTRY, and the gradient comes from autograd.

    focal_ref(case, alpha, gamma, cls_weight, reg_weight) -> (losses f64 (F,2), d_heads f64 (F*l*w, 8A), masks)

``case`` is a dict of numpy arrays: heads f32 (F*l*w, 8A), pos / neg i64 (F,3,cap), gi i64 (F,cap), counts i32 (F,2),
gts f32 (n, >=7), gt_off i32 (F+1,), anchors f32 (l,w,A,7), plus the ints F, l, w, A.  ``masks`` = (positive, ignored) bool
(F,l,w,A).
"""
import numpy as np
import torch
import torch.nn.functional as Fn


def memberships(case):
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    positive = np.zeros((F, l, w, A), bool)
    listed = np.zeros((F, l, w, A), bool)
    for f in range(F):
        n_pos, n_neg = int(case['counts'][f, 0]), int(case['counts'][f, 1])
        for x, y, z in set(zip(*(case['pos'][f, j, :n_pos].tolist() for j in range(3)))):
            positive[f, x, y, z] = True
        for x, y, z in set(zip(*(case['neg'][f, j, :n_neg].tolist() for j in range(3)))):
            listed[f, x, y, z] = True
    return positive, listed & ~positive


def regression_targets(gt, an):
    """VoxelLoss's targets (voxelnet/Loss.py:35-40) of ground truths ``gt`` (n,7) against anchors ``an`` (n,7), xyzlwhr."""
    d = torch.sqrt(an[:, 3] ** 2 + an[:, 4] ** 2)
    return torch.stack([(gt[:, 0] - an[:, 0]) / d, (gt[:, 1] - an[:, 1]) / d, (gt[:, 2] - an[:, 2]) / an[:, 5],
                        torch.log(gt[:, 3] / an[:, 3]), torch.log(gt[:, 4] / an[:, 4]), torch.log(gt[:, 5] / an[:, 5]),
                        gt[:, 6] - an[:, 6]], dim=1)


def focal_ref(case, alpha=0.25, gamma=2.0, cls_weight=1.0, reg_weight=2.0):
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    positive, ignored = memberships(case)
    negative = ~positive & ~ignored
    heads = torch.from_numpy(np.asarray(case['heads'], np.float64)).reshape(F, l, w, 8 * A).requires_grad_(True)
    anchors = torch.from_numpy(np.asarray(case['anchors'], np.float64)).reshape(l, w, A, 7)
    gts = torch.from_numpy(np.asarray(case['gts'], np.float64))
    losses = []
    for f in range(F):
        x = heads[f, :, :, :A]
        log_p, log_q = Fn.logsigmoid(x), Fn.logsigmoid(-x)            # log p, log(1 - p)
        pos_term = alpha * torch.exp(gamma * log_q) * (-log_p)
        neg_term = (1.0 - alpha) * torch.exp(gamma * log_p) * (-log_q)
        n_pos = int(case['counts'][f, 0])
        cls = cls_weight / max(1, n_pos) * (pos_term[torch.from_numpy(positive[f])].sum()
                                            + neg_term[torch.from_numpy(negative[f])].sum())
        reg = torch.zeros((), dtype=torch.float64)
        if n_pos > 0:
            px, py, pz = (torch.from_numpy(case['pos'][f, j, :n_pos].astype(np.int64)) for j in range(3))
            g = gts[int(case['gt_off'][f]) + torch.from_numpy(case['gi'][f, :n_pos].astype(np.int64)), :7]
            t = regression_targets(g, anchors[px, py, pz])
            r = heads[f, :, :, A:].reshape(l, w, A, 7)[px, py, pz]
            reg = reg_weight * Fn.smooth_l1_loss(r, t, reduction='sum', beta=1.0) / (n_pos * 7)
        losses.append(torch.stack([cls, reg]))
    losses = torch.stack(losses)
    losses.sum().backward()
    return losses.detach(), heads.grad.reshape(F * l * w, 8 * A), (positive, ignored)
