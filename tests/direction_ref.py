"""Float64 restatement of the direction classifier and the sine angle loss (include/mvx_hip.h mvx_focal_loss_dir_frames /
mvx_detect_frames_dir), built on focal_ref.py and detect_ref.py by import.

    direction_ref(case, ..., direction=True, dir_weight, dir_offset)
        -> (losses f64 (F,3), d_heads f64 (F*l*w, 8A), d_dir f64 (F*l*w, A), masks)      gradients in closed form
    direction_autograd(case, ...) -> the same losses and gradients from torch.autograd on a float64 restatement
    fold_yaw / decode_dir                                                                 the decode of section 4

``case`` is a focal_ref case plus ``dir`` f32 (F*l*w, A), the direction logits.  The classification term is focal_ref's own
(called, not restated); with ``direction=False`` the whole result is focal_ref's.
"""
import math

import numpy as np
import torch
import torch.nn.functional as Fn

import detect_ref as D
import focal_ref as R


def direction_bit(g6, dir_offset):
    """b = floor(mod(g6 - dir_offset, 2 pi) / pi) in {0, 1}, mod in [0, 2 pi)."""
    return np.floor(np.mod(np.asarray(g6, np.float64) - dir_offset, 2.0 * math.pi) / math.pi).astype(np.int64) % 2


def _entries(case, f):
    """The pos_idx entries of frame f that the regression term takes: (x, y, z, rows of gts), out-of-grid anchors and
    out-of-range gi skipped, duplicates kept."""
    l, w, A = case['l'], case['w'], case['A']
    n_pos = int(case['counts'][f, 0])
    px, py, pz = (case['pos'][f, j, :n_pos].astype(np.int64) for j in range(3))
    gi = case['gi'][f, :n_pos].astype(np.int64)
    n_gt = int(case['gt_off'][f + 1]) - int(case['gt_off'][f])
    ok = (px >= 0) & (px < l) & (py >= 0) & (py < w) & (pz >= 0) & (pz < A) & (gi >= 0) & (gi < n_gt)
    return px[ok], py[ok], pz[ok], int(case['gt_off'][f]) + gi[ok], n_pos


def direction_ref(case, alpha=0.25, gamma=2.0, cls_weight=1.0, reg_weight=2.0, direction=True, dir_weight=0.2,
                  dir_offset=math.pi / 4):
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    plain = R.focal_ref(case, alpha, gamma, cls_weight, reg_weight)
    if not direction:
        return plain
    losses = torch.zeros((F, 3), dtype=torch.float64)
    losses[:, 0] = plain[0][:, 0]
    d_heads = np.zeros((F, l, w, 8 * A))
    d_heads[..., :A] = plain[1].reshape(F, l, w, 8 * A)[..., :A].numpy()        # the classification term: focal_ref's own
    d_dir = np.zeros((F, l, w, A))
    heads = np.asarray(case['heads'], np.float64).reshape(F, l, w, 8 * A)
    logits = np.asarray(case['dir'], np.float64).reshape(F, l, w, A)
    anchors = torch.from_numpy(np.asarray(case['anchors'], np.float64)).reshape(l, w, A, 7)
    gts = np.asarray(case['gts'], np.float64)
    for f in range(F):
        px, py, pz, rows, n_pos = _entries(case, f)
        if n_pos == 0:
            continue
        g = gts[rows, :7]
        t = R.regression_targets(torch.from_numpy(g), anchors[px, py, pz]).numpy()
        r = heads[f, :, :, A:].reshape(l, w, A, 7)[px, py, pz]
        diff = r - t
        chain = np.ones_like(diff)
        chain[:, 6] = np.cos(diff[:, 6])                       # the angle through its sine
        diff[:, 6] = np.sin(diff[:, 6])
        ad = np.abs(diff)
        reg_scale = reg_weight / (n_pos * 7)
        losses[f, 1] = reg_scale * float(np.where(ad < 1.0, 0.5 * diff * diff, ad - 0.5).sum())
        grad = reg_scale * np.where(ad < 1.0, diff, np.sign(diff)) * chain
        x = logits[f][px, py, pz]
        b = direction_bit(g[:, 6], dir_offset)
        dir_scale = dir_weight / max(1, n_pos)
        sp = np.maximum(np.where(b == 1, -x, x), 0.0) + np.log1p(np.exp(-np.abs(x)))      # softplus(-x) : softplus(x)
        losses[f, 2] = dir_scale * float(sp.sum())
        gdir = dir_scale * (1.0 / (1.0 + np.exp(-x)) - b)
        for k in range(px.shape[0]):                           # entries that name an anchor twice add up
            d_heads[f, px[k], py[k], A + pz[k] * 7:A + pz[k] * 7 + 7] += grad[k]
            d_dir[f, px[k], py[k], pz[k]] += gdir[k]
    return (losses, torch.from_numpy(d_heads.reshape(F * l * w, 8 * A)), torch.from_numpy(d_dir.reshape(F * l * w, A)), plain[2])


def direction_autograd(case, alpha=0.25, gamma=2.0, cls_weight=1.0, reg_weight=2.0, dir_weight=0.2, dir_offset=math.pi / 4):
    """The same contract written forward only, in float64 torch; the gradients come from autograd."""
    F, l, w, A = case['F'], case['l'], case['w'], case['A']
    positive, ignored = R.memberships(case)
    negative = ~positive & ~ignored
    heads = torch.from_numpy(np.asarray(case['heads'], np.float64)).reshape(F, l, w, 8 * A).requires_grad_(True)
    logits = torch.from_numpy(np.asarray(case['dir'], np.float64)).reshape(F, l, w, A).requires_grad_(True)
    anchors = torch.from_numpy(np.asarray(case['anchors'], np.float64)).reshape(l, w, A, 7)
    gts = torch.from_numpy(np.asarray(case['gts'], np.float64))
    losses = []
    for f in range(F):
        x = heads[f, :, :, :A]
        log_p, log_q = Fn.logsigmoid(x), Fn.logsigmoid(-x)
        px, py, pz, rows, n_pos = _entries(case, f)
        cls = cls_weight / max(1, n_pos) * ((alpha * torch.exp(gamma * log_q) * -log_p)[torch.from_numpy(positive[f])].sum()
                                            + ((1.0 - alpha) * torch.exp(gamma * log_p) * -log_q)[torch.from_numpy(negative[f])].sum())
        reg = dirl = torch.zeros((), dtype=torch.float64)
        if n_pos > 0:
            g = gts[torch.from_numpy(rows), :7]
            t = R.regression_targets(g, anchors[px, py, pz])
            r = heads[f, :, :, A:].reshape(l, w, A, 7)[px, py, pz]
            pred = torch.cat([r[:, :6], torch.sin(r[:, 6:] - t[:, 6:])], dim=1)
            want = torch.cat([t[:, :6], torch.zeros_like(t[:, 6:])], dim=1)
            reg = reg_weight * Fn.smooth_l1_loss(pred, want, reduction='sum', beta=1.0) / (n_pos * 7)
            b = torch.from_numpy(direction_bit(g[:, 6].numpy(), dir_offset)).double()
            dirl = dir_weight / max(1, n_pos) * Fn.binary_cross_entropy_with_logits(logits[f][px, py, pz], b, reduction='sum')
        losses.append(torch.stack([cls, reg, dirl]))
    losses = torch.stack(losses)
    losses.sum().backward()
    return losses.detach(), heads.grad.reshape(F * l * w, 8 * A), logits.grad.reshape(F * l * w, A)


# ---- decode ---------------------------------------------------------------------------------------------------------------
def wrap_pi(t):
    """Into [-pi, pi)."""
    t = np.asarray(t, np.float64)
    return t - np.floor((t + math.pi) / (2.0 * math.pi)) * (2.0 * math.pi)


def fold_yaw(theta, logit, dir_offset):
    """The decoded yaw folded into the half turn the direction logit names, in [-pi, pi)."""
    v = np.asarray(theta, np.float64) - dir_offset
    base = v - np.floor(v / math.pi) * math.pi
    return wrap_pi(base + dir_offset + math.pi * (np.asarray(logit) > 0))


def decode_dir(reg, anchors, logits, dir_offset, mode='loss'):
    """detect_ref.decode, then the fold."""
    out = D.decode(reg, anchors, mode)
    out[:, 6] = fold_yaw(out[:, 6], logits, dir_offset)
    return out


def fold_margin(theta, dir_offset):
    """Distance of mod(theta - dir_offset, pi) from 0 and pi: where the f32 device and this reference may differ."""
    m = np.mod(np.asarray(theta, np.float64) - dir_offset, math.pi)
    return np.minimum(m, math.pi - m)
