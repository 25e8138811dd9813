"""Inputs of the ignore-pass tests (tests/test_ignore_host.py, tests/test_ignore_gpu.py): a camera, small anchor grids (those of
tests/targets_cases.py and two of their kind over other ranges), rectangles, look-alike boxes and a point-count fixture.
Everything is numpy; cached results are shared and not modified by the callers."""
import functools

import numpy as np

import mvx_oracle as O
import targets_cases as C

NEG, POS, FORCE = 0.45, 0.6, 0.1
# ioa_thr of the tests.  Not the default 0.5: one anchor of the 24x20 grid is covered by the truck of grid_gts to 0.50004 of its
# area, which would leave that decision to the rounding of the clipping.  At 0.45 the nearest pair of the fixtures is 2e-3 of the
# anchor's area away (at 0.25, 0.7 and 0.9, the other thresholds used, at least 4e-4); the GPU tests assert it on their own tables.
IOA = 0.45

# a standard KITTI P2, an identity R0 and an axis swap Tr (camera x = -y, y = -z, z = x of the LiDAR) with translation (0, -0.08, -0.27)
P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
TR = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, -0.08], [1.0, 0.0, 0.0, -0.27], [0.0, 0.0, 0.0, 1.0]])
MATRIX = P2 @ TR                                    # (3, 4) float64: LiDAR -> image

RECT_A = [560.0, 150.0, 700.0, 230.0]
RECT_B = [300.0, 170.0, 420.0, 200.0]
RECT_ALL = [0.0, 0.0, 1242.0, 375.0]
RECTS = {                                           # per grid: rectangles that hold a part of its anchor centres
    '24x20x2': [RECT_A, RECT_B], '12x10x3': [[300.0, 170.0, 380.0, 177.5]], '16x12x1': [[500.0, 180.0, 700.0, 186.0]],
    '44x50x2': [RECT_A], '24x20x2behind': [RECT_ALL],
}

EXTRA_GRIDS = {                                     # name: (l, w, A, range)
    '44x50x2': (44, 50, 2, [0.0, -20.0, -3.0, 35.2, 20.0, 1.0]),          # 4,400 anchors: 18 blocks of 256
    '24x20x2behind': (24, 20, 2, [-8.0, -4.0, -3.0, 1.6, 4.0, 1.0]),      # starts behind the camera
}


@functools.lru_cache(maxsize=None)
def grid(name):
    """targets_cases.grid, or one of EXTRA_GRIDS in the same form."""
    if name not in EXTRA_GRIDS:
        return C.grid(name)
    l, w, A, rng = EXTRA_GRIDS[name]
    an = O.create_anchors(l, w, rng, O.CARSIZE).reshape(l, w, 2, 7).contiguous()
    return dict(l=l, w=w, A=A, rng=rng, anchors=an.numpy(), bevs=O.bbox3d2bev(an).numpy())


def base_boxes(name='24x20x2'):
    """(Cars (9, 7), look-alikes (2, 7)) of the base case: grid_gts without its truck row as Cars; the truck and a 5.0 x 2.0 m van
    at yaw 0.3 between two cars as look-alike boxes."""
    gt = C.grid_gts(name)
    g = grid(name)
    rng = g['rng']
    xm, ym = 0.5 * (rng[0] + rng[3]), 0.5 * (rng[1] + rng[4])
    van = np.array([[xm + 1.0, ym - 3.0, -1.0, 5.0, 2.0, 2.2, 0.3]], np.float32)      # between the two cars of the y0 corners
    return gt[:9].copy(), np.concatenate([van, gt[9:10]])


def cars_for(name, n, seed):
    return C.many_gts(name, n, seed) if name not in EXTRA_GRIDS else _many(grid(name), n, seed)


def _many(g, n, seed):
    rng, r = g['rng'], np.random.default_rng(seed)
    gt = np.zeros((n, 7), np.float32)
    gt[:, 0] = r.uniform(rng[0] + 0.2, rng[3] - 0.2, n)
    gt[:, 1] = r.uniform(rng[1] + 0.2, rng[4] - 0.2, n)
    gt[:, 2] = -1.0
    gt[:, 3:6] = np.array([3.9, 1.6, 1.56]) * r.uniform(0.9, 1.1, (n, 3))
    gt[:, 6] = r.integers(0, 2, n) * (np.pi / 2) + r.uniform(-0.1, 0.1, n)
    return gt


def orientations(g, A):
    """The grid ``g`` cut to its first A orientations, or with a third one at pi/4 (A = 3): dict as targets_cases.grid."""
    import torch
    if A == g['A']:
        return g
    an = torch.from_numpy(g['anchors'])
    if A < g['A']:
        an = an[:, :, :A]
    else:
        third = an[:, :, :1].clone()
        third[..., 6] = torch.pi / 4
        an = torch.cat([an, third], dim=2)
    an = an.contiguous()
    return dict(l=g['l'], w=g['w'], A=A, rng=g['rng'], anchors=an.numpy(), bevs=O.bbox3d2bev(an).numpy())


@functools.lru_cache(maxsize=None)
def point_fixture():
    """Three frames, rotated boxes, 3,000 / 2,200 / 1 valid rows of 3,072 (three workgroups of 1,024 rows share a box); the rows
    beyond n_points are filled with points INSIDE a box, which a kernel that reads them would count.
    dict(points f32 (3, 3072, 6), n_points i32 (3,), boxes f32 (G, 7), gt_off i32 (4,))."""
    r = np.random.default_rng(41)
    cap = 3072
    boxes = np.array([[12.0, 1.0, -1.6, 3.9, 1.6, 1.5, 0.3], [20.0, -3.0, -1.7, 4.2, 1.7, 1.6, -1.2], [8.0, 4.0, -1.5, 10.0, 2.6, 3.0, 2.5],
                      [15.0, 0.0, -1.6, 3.9, 1.6, 1.5, 1.5707964], [30.0, 5.0, -1.0, 0.8, 0.7, 1.8, 0.7],
                      [25.0, -6.0, -1.6, 3.9, 1.6, 1.5, -3.0]], np.float32)
    gt_off = np.array([0, 3, 5, 6], np.int32)
    n_points = np.array([3000, 2200, 1], np.int32)
    pts = np.zeros((3, cap, 6), np.float32)
    for f in range(3):
        own = boxes[gt_off[f]:gt_off[f + 1]]
        n = int(n_points[f])
        scene = np.stack([r.uniform(0.0, 40.0, cap), r.uniform(-10.0, 10.0, cap), r.uniform(-2.0, 1.0, cap)], axis=1)
        # two thirds of the valid rows around the frame's boxes (inside and just outside them), spread over all rows
        which = r.integers(0, len(own), cap)
        b = own[which]
        u = r.uniform(-0.6, 0.6, cap) * b[:, 3]
        v = r.uniform(-0.6, 0.6, cap) * b[:, 4]
        c, s = np.cos(b[:, 6].astype(np.float64)), np.sin(b[:, 6].astype(np.float64))
        near = np.stack([b[:, 0] + u * c + v * s, b[:, 1] - u * s + v * c, b[:, 2] + r.uniform(-0.2, 1.2, cap) * b[:, 5]], axis=1)
        pick = r.random(cap) < 0.67
        pts[f, :, :3] = np.where(pick[:, None], near, scene)
        pts[f, n:, :3] = own[0, :3] + np.array([0.0, 0.0, 0.5 * own[0, 5]], np.float32)      # the box centre: inside
        pts[f, 0, :3] = own[0, :3] + np.array([0.1, 0.1, 0.3 * own[0, 5]], np.float32)         # the first row: inside as well
        pts[f, :, 3:] = r.uniform(0.0, 1.0, (cap, 3))
    return dict(points=pts, n_points=n_points, boxes=boxes, gt_off=gt_off)
