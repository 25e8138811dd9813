"""Inputs of the direct label-path tests (tests/test_targets_direct_host.py, tests/test_targets_direct_gpu.py): BEV box pairs
in the configurations where a clipping goes wrong, small anchor grids over ranges that are not KITTI's, ground truths for
them, and VoxelLoss cases.  Everything is numpy; the loss cases follow the layout of targets_ref.voxel_loss64.

IoU tolerance (IOU_BOUND, INTER_BOUND).  The reference-arithmetic oracle (oracle/anchors_c.c, one pair per call) against the
float64 truth targets_ref.poly_iou64 on the CLEAN pairs of box_pairs() -- the pairs on which the oracle never consumes a
stale scratch slot -- measured on the CPU:
    max |IoU_oracle - IoU_truth|     = 7.4e-5   (MEASURED_IOU;   a random pair 75 m from the origin)
    max |inter_oracle - inter_truth| = 3.9e-4   (MEASURED_INTER, m^2; the same pair)
The bounds are 4x those figures rounded up to one significant digit, IOU_BOUND = 3e-4 and INTER_BOUND = 2e-3 m^2;
tests/test_targets_direct_host.py asserts the measurement (the oracle stays inside the bounds on every clean pair) and the
derivation (bound = 4x, one digit).  The error grows with the distance from the origin, about which the clipping fans: at
(70, 39) the cross products reach 5,000 m^2, where one f32 ulp is 5e-4 m^2; within 40 m it stays below 1e-5.
On the GPU (MI355X) mvx_bbox_pairwise is bit-equal to the oracle on the clean pairs, so its largest error there is the same;
on the 12 stale pairs, where it fills the degenerate slot with the edge's start point, its largest error is 4.7e-8 (IoU) and
8.4e-6 m^2 (intersection)."""
import functools

import numpy as np

import mvx_oracle as O

MEASURED_IOU = 7.4e-5
MEASURED_INTER = 3.9e-4
IOU_BOUND = 3e-4
INTER_BOUND = 2e-3

PLACEMENTS = {'origin': (2.0, 1.0), 'mid': (35.0, 0.0), 'far': (70.0, 39.0)}
GARBAGE = 10 ** 9
MANY_SEED = 7                                 # of the 600 ground truths of the two-trip concatenation case


def rect(cx, cy, l, w):
    """Axis-aligned l x w box, counter-clockwise from (+,+): the corner order of bbox3d2bev at yaw 0."""
    hl, hw = l / 2.0, w / 2.0
    return np.array([[cx + hl, cy + hw], [cx - hl, cy + hw], [cx - hl, cy - hw], [cx + hl, cy - hw]], np.float32)


def diamond(cx, cy, r):
    """A square of half diagonal r turned by 45 degrees: corners on the axes through its centre, exact in f32."""
    return np.array([[cx + r, cy], [cx, cy + r], [cx - r, cy], [cx, cy - r]], np.float32)


def _placed(name, build):
    return [('%s@%s' % (name, tag), *build(x, y)) for tag, (x, y) in PLACEMENTS.items()]


_LEFTOVER = (
    ([[62.14143753051758, 3.745983839035034], [9.022642135620117, 3.745983839035034], [9.022642135620117, 1.5244856967910891e-06],
      [62.14143753051758, 3.3361634450557176e-06]],
     [[0.5, 0.5661783814430237], [0.5, 0.0], [58.60764694213867, 0.0], [58.60764694213867, 0.5661783814430237]]),
    ([[50.06527328491211, 3.590035646539036e-07], [50.06527328491211, 3.0057125091552734], [9.779019355773926, 3.0057125091552734],
      [9.779019355773926, 1.708686028223383e-07]],
     [[58.16537857055664, 2.037842035293579], [4.0, 2.037842035293579], [4.0, 0.0], [58.16537857055664, 0.0]]),
    ([[15.292672157287598, 1.7633999586105347], [15.292672157287598, 4.168986436070554e-07], [49.03650665283203, 6.96357687957061e-07],
      [49.03650665283203, 1.7633999586105347]],
     [[2.0, 2.875190258026123], [2.0, 0.0], [37.03755187988281, 0.0], [37.03755187988281, 2.875190258026123]]),
    ([[53.62776565551758, 3.939673900604248], [31.457853317260742, 3.939673900604248], [31.457853317260742, 1.4452566574618686e-06],
      [53.62776565551758, 2.4017256237129914e-06]],
     [[26.79490089416504, 4.267383575439453], [0.5, 4.267383575439453], [0.5, 0.0], [26.79490089416504, 0.0]]),
)


@functools.lru_cache(maxsize=None)
def box_pairs():
    """[(name, quad a (4,2) f32, quad b (4,2) f32)].  Degenerate configurations use coordinates that are multiples of 2^-2, so
    shared edges and touching corners are exact in f32 at every placement."""
    sliver, gap = np.float32(1e-4), np.float32(1e-3)
    t = []
    t += _placed('identical', lambda x, y: (rect(x, y, 4, 2), rect(x, y, 4, 2)))
    t += _placed('shared_full_edge', lambda x, y: (rect(x, y, 4, 2), rect(x + 4, y, 4, 2)))
    t += _placed('shared_partial_edge', lambda x, y: (rect(x, y, 4, 2), rect(x + 4, y + 1, 4, 2)))
    t += _placed('corner_touches_corner', lambda x, y: (rect(x, y, 4, 2), rect(x + 4, y + 2, 4, 2)))
    t += _placed('corner_on_edge', lambda x, y: (rect(x, y, 4, 2), diamond(x + 3, y, 1)))
    t += _placed('corner_on_edge_inside', lambda x, y: (rect(x, y, 4, 2), diamond(x + 1, y, 1)))
    t += _placed('one_inside_the_other', lambda x, y: (rect(x, y, 4, 2), rect(x + 0.25, y, 2, 1)))
    t += _placed('cross_0_over_90', lambda x, y: (rect(x, y, 4, 2), np.roll(rect(x, y, 2, 4), 1, axis=0)))
    t += _placed('45_over_0', lambda x, y: (diamond(x, y, 1.5), rect(x, y, 4, 2)))
    t += _placed('sliver_1e-4', lambda x, y: (rect(x, y, 4, 2), rect(x + 4 - sliver, y, 4, 2)))
    t += _placed('disjoint_1mm', lambda x, y: (rect(x, y, 4, 2), rect(x + 4 + gap, y, 4, 2)))
    t += _placed('clockwise_first', lambda x, y: (rect(x, y, 4, 2)[::-1].copy(), rect(x + 1, y + 0.5, 4, 2)))
    t += _placed('clockwise_second', lambda x, y: (rect(x, y, 4, 2), rect(x + 1, y + 0.5, 4, 2)[::-1].copy()))
    t += _placed('clockwise_both', lambda x, y: (rect(x, y, 4, 2)[::-1].copy(), diamond(x + 1, y, 1.5)[::-1].copy()))
    # the clipping is a fan about the ORIGIN: boxes that own it, touch it or have an edge through it
    through = rect(2, 0, 4, 2)                          # its edge x = 0 passes through the origin
    corner = rect(2, 1, 4, 2)                           # its corner (0, 0)
    holds = rect(0.5, 0.25, 4, 2)                       # the origin inside
    for name, box in (('edge_through_origin', through), ('corner_at_origin', corner), ('contains_origin', holds)):
        t.append((name + '/itself', box, box.copy()))
        t.append((name + '/shifted', box, box + np.float32([1.0, 0.5])))
        t.append((name + '/diamond', box, diamond(0.5, 0.5, 1.5)))
        t.append((name + '/diamond_at_origin', box, diamond(0, 0, 1)))
        t.append((name + '/swapped', diamond(0.5, 0.5, 1.5), box))
    for k, (x, y) in enumerate(((8.0, 8.0), (35.0, 35.0), (64.0, 32.0))):          # edges ON a line through the origin
        t.append(('radial_edges/%d' % k, diamond(x, y, 2), diamond(x + 1, y + 1, 2)))
        t.append(('radial_shared_edge/%d' % k, diamond(x, y, 2), diamond(x + 2, y + 2, 2)))
    # The degenerate crossing of cut(): an edge of the first box runs ALONG the fan line from the origin to a corner (cx, 0) of
    # the second, a few 1e-6 / cx off it, so its end points fall on different sides of the 1e-6 tolerance (s1 = cx * y1 counts
    # as 0, s2 = cx * y2 as positive) while |s2 - s1| <= 1e-6: the reference consumes a scratch slot without writing it.
    for k, (cx, y1, y2, far) in enumerate(((0.5, 1.5e-6, 3.2e-6, 40.5), (0.5, 1.5e-6, 3.2e-6, 2.5), (0.25, 3e-6, 6.5e-6, 40.25),
                                           (1.0, 0.7e-6, 1.6e-6, 3.0), (2.0, 0.35e-6, 0.8e-6, 50.0), (0.5, 1.25e-6, 3e-6, 64.5),
                                           (4.0, 0.15e-6, 0.4e-6, 36.0), (0.125, 6e-6, 13e-6, 45.125))):
        a = np.array([[60.0, 2.0], [30.0, 2.0], [30.0, y1], [60.0, y2]], np.float32)
        b = np.array([[far, 3.0], [cx, 3.0], [cx, 0.0], [far, 0.0]], np.float32)
        t.append(('along_fan_line/%d' % k, a, b))
        t.append(('along_fan_line/%d/mirrored' % k, a[::-1, ::-1].copy(), b[::-1, ::-1].copy()))
    # ... and four of that family (found by a seeded search) in which the content of the consumed slot MATTERS: with the edge's
    # start point in it the result is right to 1e-5 m^2; with what the slot held from the previous cut it is off by 7e-3 to
    # 0.28 m^2.  (The walk's rotation of the corners and the roles of the two boxes differ from the eight above.)
    for k, (a, b) in enumerate(_LEFTOVER):
        t.append(('along_fan_line_leftover/%d' % k, np.array(a, np.float32), np.array(b, np.float32)))
    rng = np.random.default_rng(11)
    for k in range(64):                                 # anchor-scale boxes anywhere in the KITTI range, partner nearby
        g = np.zeros((2, 7), np.float32)
        g[0, :2] = rng.uniform((0.0, -40.0), (70.4, 40.0))
        g[1, :2] = g[0, :2] + rng.normal(0.0, 1.2, 2)
        g[:, 3:5] = np.array([3.9, 1.6]) * rng.uniform(0.8, 1.25, (2, 2))
        g[:, 6] = rng.uniform(-np.pi, np.pi, 2)
        q = bev(g)
        t.append(('random/%d' % k, q[0], q[1]))
    return t


def pair_arrays():
    t = box_pairs()
    return [n for n, _, _ in t], np.stack([a for _, a, _ in t]), np.stack([b for _, _, b in t])


def oracle_pair(a, b):
    """(IoU, intersection, stale reads) of ONE pair from the oracle: a call of its own, so no other pair's history."""
    lib = O._oracle_c()
    before = lib.oracle_anchor_stale_reads()
    iou = O.bbox_pairwise(a[None], b[None], True)[0, 0]
    inter = O.bbox_pairwise(a[None], b[None], False)[0, 0]
    return iou, inter, lib.oracle_anchor_stale_reads() - before


@functools.lru_cache(maxsize=None)
def pair_table():
    """Per pair of box_pairs(): (name, oracle IoU f32, oracle intersection f32, stale reads, true IoU, true intersection).
    Computed once and shared; callers do not modify it."""
    import targets_ref as R
    rows = []
    for n, a, b in box_pairs():
        iou, inter, stale = oracle_pair(a, b)
        t_inter, t_iou = R.poly_iou64(a, b)
        rows.append((n, iou, inter, stale, t_iou, t_inter))
    return rows


def random_pairs(n, seed):
    """n seeded pairs for the bounding-circle test: sizes 0.5..12 m, any yaw, centre distances spread around the sum of the
    two radii (a third of them further apart than the circles reach)."""
    rng = np.random.default_rng(seed)
    g = np.zeros((2, n, 7), np.float32)
    g[:, :, 3:5] = rng.uniform(0.5, 12.0, (2, n, 2))
    g[:, :, 6] = rng.uniform(-np.pi, np.pi, (2, n))
    g[0, :, :2] = rng.uniform((0.0, -40.0), (70.4, 40.0), (n, 2))
    reach = 0.5 * (np.hypot(g[0, :, 3], g[0, :, 4]) + np.hypot(g[1, :, 3], g[1, :, 4]))
    phi = rng.uniform(-np.pi, np.pi, n)
    dist = reach * rng.uniform(0.6, 1.3, n)
    g[1, :, 0] = g[0, :, 0] + dist * np.cos(phi)
    g[1, :, 1] = g[0, :, 1] + dist * np.sin(phi)
    return bev(g[0]), bev(g[1])


def bev(boxes7):
    import torch
    return O.bbox3d2bev(torch.from_numpy(np.ascontiguousarray(boxes7, np.float32))).numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# small anchor grids
# ---------------------------------------------------------------------------------------------------------------------------
GRIDS = {                                     # name: (l, w, A, range)
    '24x20x2': (24, 20, 2, [10.0, -4.0, -3.0, 19.6, 4.0, 1.0]),
    '16x12x1': (16, 12, 1, [5.0, -2.4, -3.0, 11.4, 2.4, 1.0]),
    '12x10x3': (12, 10, 3, [20.0, 6.0, -3.0, 24.8, 10.0, 1.0]),
    '120x60x2': (120, 60, 2, [30.0, -3.0, -3.0, 42.0, 3.0, 1.0]),          # 0.1 m cells: the walk needs R = 55
    '120x60x2thin': (120, 60, 2, [30.0, -3.0, -3.0, 42.0, 3.0, 1.0]),      # ... with 4.0 x 0.4 m anchors (THIN_SIZE)
}
THIN_SIZE = [4.0, 0.4, 1.5]


@functools.lru_cache(maxsize=None)
def grid(name):
    """dict(l, w, A, rng, anchors f32 (l,w,A,7), bevs f32 (l,w,A,4,2)).  A = 1: yaw 0; A = 2: yaw 0, pi/2 (create_anchors);
    A = 3: yaw 0, pi/2, pi/4 -- all of the same Car size."""
    import torch
    l, w, A, rng = GRIDS[name]
    two = O.create_anchors(l, w, rng, THIN_SIZE if name.endswith('thin') else O.CARSIZE).reshape(l, w, 2, 7)
    if A == 1:
        an = two[:, :, :1]
    elif A == 2:
        an = two
    else:
        third = two[:, :, :1].clone()
        third[..., 6] = torch.pi / 4
        an = torch.cat([two, third], dim=2)
    an = an.contiguous()
    return dict(l=l, w=w, A=A, rng=rng, anchors=an.numpy(), bevs=O.bbox3d2bev(an).numpy())


def centre_cells(g, gt7):
    import torch
    nls, nws = O.anchor_center_cells(torch.from_numpy(np.ascontiguousarray(gt7[:, :2], np.float32)), (g['l'], g['w']), g['rng'])
    return nls.numpy(), nws.numpy()


def grid_gts(name):
    """Ground truths (n,7) for a grid: its four corners, its centre, a box exactly equal to an anchor and the same box again,
    yaw +-pi/4, and a truck-sized box."""
    g = grid(name)
    rng = g['rng']
    cl, cw = (rng[3] - rng[0]) / g['l'], (rng[4] - rng[1]) / g['w']
    x0, x1, y0, y1 = rng[0] + 0.3 * cl, rng[3] - 0.3 * cl, rng[1] + 0.3 * cw, rng[4] - 0.3 * cw
    xm, ym = 0.5 * (rng[0] + rng[3]) + 0.13, 0.5 * (rng[1] + rng[4]) - 0.07
    car = [3.9, 1.6, 1.56]
    an = g['anchors'][g['l'] // 3, g['w'] // 3, 0]
    rows = [[x0, y0, -1.0] + car + [0.03], [x0, y1, -1.0] + car + [1.55], [x1, y0, -1.0] + car + [-0.02],
            [x1, y1, -1.0] + car + [1.6], [xm, ym, -1.0] + car + [0.05], list(an), list(an),
            [xm + 1.1, ym + 0.4, -1.0] + car + [np.pi / 4], [xm - 1.3, ym - 0.6, -1.0] + car + [-np.pi / 4],
            [xm + 0.2, ym + 0.3, -1.0, 10.0, 2.6, 3.0, 0.2]]
    return np.array(rows, np.float32)


def thin_gts():
    """For '120x60x2thin': one ground truth of the anchors' own 4.0 x 0.4 m shape, 0.04 m ahead of an anchor centre.  The anchor
    32 cells further on is 3.24 m away: IoU 0.76 / 7.24 = 0.105, still part of the walk, while the two bounding circles (radii
    2.01 m) nearly touch -- the pair that a too eager bounding-circle test would drop."""
    g = grid('120x60x2thin')
    an = g['anchors'][40, 30, 0].copy()
    an[0] -= np.float32(0.04)
    return an[None]


def many_gts(name, n, seed):
    """n Car-sized ground truths, yaw near 0 or pi/2, scattered over the grid."""
    g = grid(name)
    rng, r = g['rng'], np.random.default_rng(seed)
    gt = np.zeros((n, 7), np.float32)
    gt[:, 0] = r.uniform(rng[0] + 0.2, rng[3] - 0.2, n)
    gt[:, 1] = r.uniform(rng[1] + 0.2, rng[4] - 0.2, n)
    gt[:, 2] = -1.0
    gt[:, 3:6] = np.array([3.9, 1.6, 1.56]) * r.uniform(0.9, 1.1, (n, 3))
    gt[:, 6] = r.integers(0, 2, n) * (np.pi / 2) + r.uniform(-0.1, 0.1, n)
    return gt


# ---------------------------------------------------------------------------------------------------------------------------
# VoxelLoss cases
# ---------------------------------------------------------------------------------------------------------------------------
LOSS_GRIDS = {'5x7x2': (5, 7, 2), '16x12x1': (16, 12, 1), '12x10x3': (12, 10, 3), '32x32x2': (32, 32, 2)}


def loss_anchors(L, W, A):
    """f32 (L,W,A,7): a 0.4 m grid of Car anchors, yaw k * pi / A."""
    an = np.zeros((L, W, A, 7), np.float32)
    an[..., 0] = (np.arange(L, dtype=np.float32) * 0.4 + 0.2)[:, None, None]
    an[..., 1] = (np.arange(W, dtype=np.float32) * 0.4 - 0.2 * W)[None, :, None]
    an[..., 2] = -1.0
    an[..., 3:6] = np.array([3.9, 1.6, 1.56], np.float32)
    an[..., 6] = (np.arange(A, dtype=np.float32) * np.float32(np.pi / A))[None, None, :]
    return an


def _triples(flat, W, A):
    flat = np.asarray(flat, np.int64)
    return np.stack([flat // (W * A), (flat // A) % W, flat % A])


def loss_case(L, W, A, n_pos, n_ign, n_gt, seed, dup=True, gt_ld=7):
    """Random scores in (0,1), regression ~ N(0, 1.2) (both SmoothL1 branches), ``n_pos`` distinct positives and ``n_ign`` more
    anchors listed as non-negative only.  With ``dup`` the first positive is listed twice (different gi) and one non-negative
    three times."""
    rng = np.random.default_rng(seed)
    N = L * W * A
    score = (1.0 / (1.0 + np.exp(-rng.normal(0.0, 2.0, (L, W, A))))).astype(np.float32)
    reg = rng.normal(0.0, 1.2, (L, W, 7 * A)).astype(np.float32)
    pick = rng.permutation(N)[:n_pos + n_ign]
    p, n = pick[:n_pos], pick[rng.permutation(n_pos + n_ign)]
    if dup and n_pos > 0:
        p = np.concatenate([p, p[:1]])
        n = np.concatenate([n, n[-1:], n[-1:]])
    gts = np.zeros((n_gt, gt_ld), np.float32)
    gts[:, 0] = rng.uniform(0.0, 0.4 * L, n_gt)
    gts[:, 1] = rng.uniform(-0.2 * W, 0.2 * W, n_gt)
    gts[:, 2] = rng.uniform(-1.6, -0.4, n_gt)
    gts[:, 3:6] = np.array([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.2, (n_gt, 3))
    gts[:, 6] = rng.uniform(-1.5, 1.5, n_gt)
    gts[:, 7:] = 1e30                                   # columns past 7 are never read
    return dict(L=L, W=W, A=A, score=score, reg=reg, pos=_triples(p, W, A), neg=_triples(n, W, A),
                gi=rng.integers(0, n_gt, p.shape[0]).astype(np.int64), gts=gts, anchors=loss_anchors(L, W, A))


@functools.lru_cache(maxsize=None)
def loss_small(name):
    """The four small grids: duplicates present, both lists short."""
    L, W, A = LOSS_GRIDS[name]
    if name == '32x32x2':                               # both lists longer than the 1024 threads of loss_lists
        return loss_case(L, W, A, 1100, 150, 9, seed=32)
    return loss_case(L, W, A, 6, 5, 3, seed=L * 100 + W)


@functools.lru_cache(maxsize=None)
def loss_gt_ld9():
    return loss_case(5, 7, 2, 6, 5, 3, seed=59, gt_ld=9)


@functools.lru_cache(maxsize=None)
def loss_no_positive():
    """n_pos = 0 with reg given; the non-negative list stays."""
    c = dict(loss_case(5, 7, 2, 0, 5, 3, seed=57, dup=False))
    return c


@functools.lru_cache(maxsize=None)
def loss_no_lists():
    c = dict(loss_case(5, 7, 2, 0, 0, 3, seed=58, dup=False))
    return c


@functools.lru_cache(maxsize=None)
def loss_all_listed():
    """n_neg = N: every anchor is listed as non-negative, the negative sum is empty (0 / eps)."""
    c = dict(loss_case(5, 7, 2, 4, 0, 3, seed=60, dup=False))
    c['neg'] = _triples(np.random.default_rng(61).permutation(5 * 7 * 2), 7, 2)
    return c


@functools.lru_cache(maxsize=None)
def loss_saturated():
    """Scores of exactly 0.0 and 1.0 among the positives, the non-negatives and the unlisted anchors."""
    c = dict(loss_case(5, 7, 2, 6, 5, 3, seed=62, dup=False))
    score = c['score'].copy()
    listed = set(map(tuple, c['neg'].T.tolist()))
    free = [xyz for xyz in np.ndindex(5, 7, 2) if xyz not in listed][:2]
    pos_only, ign_only = c['pos'].T[:2], [xyz for xyz in c['neg'].T.tolist() if xyz not in c['pos'].T.tolist()][:2]
    for (xyz0, xyz1) in (pos_only, ign_only, free):
        score[tuple(xyz0)] = 0.0
        score[tuple(xyz1)] = 1.0
    c['score'] = score
    return c


KINK = np.array([1.0, -1.0, np.nextafter(np.float32(1), np.float32(0)), -np.nextafter(np.float32(1), np.float32(0)),
                 np.nextafter(np.float32(1), np.float32(2)), -np.nextafter(np.float32(1), np.float32(2)), 0.0], np.float32)


@functools.lru_cache(maxsize=None)
def loss_kink():
    """Every ground truth equals its anchor, so every target is exactly 0, and reg holds +-1, +-nextafter(1, 0),
    +-nextafter(1, 2) and 0: diff sits on the SmoothL1 kink and one ulp to either side of it."""
    L, W, A = 5, 7, 2
    c = dict(loss_case(L, W, A, 7, 3, 7, seed=63, dup=False))
    an = c['anchors'][tuple(c['pos'])]
    c['gts'] = an.copy()
    c['gi'] = np.arange(7, dtype=np.int64)
    reg = c['reg'].reshape(L, W, A, 7).copy()
    for k in range(7):
        reg[tuple(c['pos'][:, k])] = np.roll(KINK, k)
    c['reg'] = reg.reshape(L, W, 7 * A)
    return c


@functools.lru_cache(maxsize=None)
def loss_large():
    """520 x 512 x 2 = 532,480 anchors: more than the 512 x 1024 that loss_dense covers without striding its grid."""
    return loss_case(520, 512, 2, 40, 30, 5, seed=64)
