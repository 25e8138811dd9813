"""Device time of mvx_assign_anchors_frames beside mvx_classify_anchors_frames on the same inputs: 4 frames of the
full 176 x 200 x 2 anchor grid with 15 car-sized boxes each, any heading, both with the radius Calc derives for them.  Device events
around batches of calls, the two alternating, after a warm-up of both; five rounds to show the spread."""
import os
import sys

sys.argv = sys.argv[:1]
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mvxnet-makise_amd'))
import numpy as np
import torch
import modules.config as cfg
from modules import Calc, _hip
from modules.data import Preprocessing as pre

F, N_BOX, CALLS, ROUNDS = 4, 15, 200, 5
dev = torch.device('cuda')
anchors = pre.createAnchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, cfg.velorange, cfg.carsize)
bevs = Calc.bbox3d2bev(anchors.reshape(anchors.shape[:2] + (-1, 7))).to(dev).contiguous()
gg = np.random.default_rng(11)
n = F * N_BOX
gt = np.stack([gg.uniform(8, 60, n), gg.uniform(-30, 30, n), gg.uniform(-1.8, -0.6, n), gg.uniform(3.4, 4.4, n),
               gg.uniform(1.5, 1.8, n), gg.uniform(1.4, 1.7, n), gg.uniform(-np.pi, np.pi, n)], 1)
gt = torch.tensor(gt, dtype=torch.float32)
gb = Calc.bbox3d2bev(gt)
off = [k * N_BOX for k in range(F + 1)]
nls, nws = Calc.anchorCenterCells(gt[:, [0, 1]], bevs.shape, cfg.velorange)
g_dev, nl, nw = gb.float().contiguous().to(dev), nls.to(dev), nws.to(dev)
r_ref = Calc._window_radius(gb, bevs[:2, :2].cpu())
r_new = Calc._anchor_radius(bevs)


def reference():
    return _hip.classify_anchors_frames(g_dev, off, bevs, nl, nw, 0.45, 0.6, r_ref)


def maxiou(radius=r_new):
    return _hip.assign_anchors_frames(g_dev, off, bevs, 0.45, 0.6, 0.1, radius)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(CALLS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / CALLS * 1e3


for _ in range(20):
    reference()
    maxiou()
    maxiou(r_ref)
torch.cuda.synchronize()
st_ref = int(reference()[4].item())
host = maxiou()[3].cpu()
print('%d frames x %d boxes, radius %d (reference) / %d (max-IoU); status %d / %d; positives %s / %s'
      % (F, N_BOX, r_ref, r_new, st_ref, int(host[2 * F]), reference()[3][:, 0].tolist(), host[:2 * F:2].tolist()))
rows = []
for k in range(ROUNDS):
    rows.append((timed(reference), timed(maxiou), timed(lambda: maxiou(r_ref))))
    print('round %d: classify_anchors_frames %.1f us, assign_anchors_frames %.1f us (ratio %.2f), at the reference radius %.1f us'
          % (k, rows[-1][0], rows[-1][1], rows[-1][1] / rows[-1][0], rows[-1][2]))
med = np.median(np.array(rows), axis=0)
print('median: %.1f us / %.1f us = ratio %.2f; at the reference radius %.1f us = ratio %.2f'
      % (med[0], med[1], med[1] / med[0], med[2], med[2] / med[0]))
