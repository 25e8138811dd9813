"""Device time of the ignore pass (mvx_ignore_anchors_frames) and of the point count (mvx_box_point_counts_frames) beside
mvx_assign_anchors_frames in the same run: 4 frames of the full 176 x 200 x 2 anchor grid with 15 car-sized boxes,
3 DontCare rectangles and 3 look-alike boxes each, and 20,000 points per frame.  Device events around batches of calls, the three
alternating, after a warm-up of all; five rounds to show the spread."""
import os
import sys

sys.argv = sys.argv[:1]
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mvxnet-makise_amd'))
import numpy as np
import torch
import modules.config as cfg
from modules import Calc, _hip
from modules.data import Preprocessing as pre, Synthetic

F, N_BOX, N_RECT, N_ALIKE, POINTS, CALLS, ROUNDS = 4, 15, 3, 3, 20000, 200, 5
dev = torch.device('cuda')
anchors = pre.createAnchors(cfg.voxelshape[0] // 2, cfg.voxelshape[1] // 2, cfg.velorange, cfg.carsize)
an7 = anchors.reshape(anchors.shape[:2] + (-1, 7)).float().contiguous()
bevs = Calc.bbox3d2bev(an7).to(dev).contiguous()
an7 = an7.to(dev)
gg = np.random.default_rng(11)


def boxes(n, size):
    b = np.stack([gg.uniform(8, 60, n), gg.uniform(-30, 30, n), gg.uniform(-1.8, -0.6, n)] +
                 [gg.uniform(0.9 * s, 1.1 * s, n) for s in size] + [gg.uniform(-np.pi, np.pi, n)], 1)
    return torch.tensor(b, dtype=torch.float32)


gt = boxes(F * N_BOX, (3.9, 1.6, 1.56))
alike = boxes(F * N_ALIKE, (5.0, 2.0, 2.2))
g_dev = Calc.bbox3d2bev(gt).contiguous().to(dev)
q_dev = Calc.bbox3d2bev(alike).contiguous().to(dev)
gt_dev = gt.to(dev)
off = [k * N_BOX for k in range(F + 1)]
i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
gt_off, rect_off, ign_off = i32(off), i32([k * N_RECT for k in range(F + 1)]), i32([k * N_ALIKE for k in range(F + 1)])
x1, y1 = gg.uniform(0, 1000, F * N_RECT), gg.uniform(100, 250, F * N_RECT)
rects = torch.tensor(np.stack([x1, y1, x1 + gg.uniform(40, 200, F * N_RECT), y1 + gg.uniform(20, 80, F * N_RECT)], 1), dtype=torch.float32).to(dev)
calib = Synthetic.KITTI_CALIB
mats = torch.from_numpy(np.stack([(calib['P2'] @ calib['R0_rect'] @ calib['Tr_velo_to_cam'])[:3]] * F)).to(dev)
pts = torch.zeros((F, POINTS, 6), dtype=torch.float32)
pts[..., 0].uniform_(0, 70)
pts[..., 1].uniform_(-40, 40)
pts[..., 2].uniform_(-3, 1)
pts, n_pts = pts.to(dev), i32([POINTS] * F)
radius = Calc._anchor_radius(bevs)


def assign():
    return _hip.assign_anchors_frames(g_dev, off, bevs, 0.45, 0.6, 0.1, radius)


lists = assign()
counts = _hip.box_point_counts_frames(pts, n_pts, gt_dev, gt_off)


def ignore():
    return _hip.ignore_anchors_frames(lists[0], lists[1], lists[2], lists[3][:2 * F], an7, bevs, gt_off, counts, 5, rects, rect_off, mats,
                                      q_dev, ign_off, 0.5)


def count():
    return _hip.box_point_counts_frames(pts, n_pts, gt_dev, gt_off)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(CALLS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / CALLS * 1e3


for _ in range(20):
    assign()
    ignore()
    count()
torch.cuda.synchronize()
words = ignore()[3].cpu()
print('%d frames x %d boxes, %d rectangles, %d look-alike boxes, %d points; radius %d; assigner counts %s; ignore counts %s, stats %s, status %d'
      % (F, N_BOX, N_RECT, N_ALIKE, POINTS, radius, lists[3][:2 * F].tolist(), words[:2 * F].tolist(), words[2 * F:6 * F].view(F, 4).tolist(),
         int(words[6 * F])))
rows = []
for k in range(ROUNDS):
    rows.append((timed(assign), timed(ignore), timed(count)))
    print('round %d: assign_anchors_frames %.1f us, ignore_anchors_frames %.1f us, box_point_counts_frames %.1f us (ignore + count = %.2f of assign)'
          % (k, rows[-1][0], rows[-1][1], rows[-1][2], (rows[-1][1] + rows[-1][2]) / rows[-1][0]))
med = np.median(np.array(rows), axis=0)
print('median: assign %.1f us, ignore %.1f us, count %.1f us; ignore + count = %.2f of assign' % (med[0], med[1], med[2], (med[1] + med[2]) / med[0]))
