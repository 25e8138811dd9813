"""Inputs of the max-IoU assigner tests (tests/test_assign_host.py, tests/test_assign_gpu.py): the small grids and ground truths
of tests/targets_cases.py, with their IoU tables computed once and shared (callers do not modify them)."""
import functools

import numpy as np

import mvx_oracle as O
import targets_cases as C
import targets_ref as R
import assign_ref as AR

NEG, POS, FORCE = 0.45, 0.6, 0.1
CASES = {                                          # name: (grid, ground truths)
    '24x20x2': ('24x20x2', lambda: C.grid_gts('24x20x2')),
    '16x12x1': ('16x12x1', lambda: C.grid_gts('16x12x1')),
    '12x10x3': ('12x10x3', lambda: C.grid_gts('12x10x3')),
    '24x20x2many': ('24x20x2', lambda: C.many_gts('24x20x2', 12, 3)),
}
GRID_CASES = ['24x20x2', '16x12x1', '12x10x3']
FRAME_SIZES = [3, 0, 1, 0, 0, 7, 2, 0, 1, 1, 0, 4, 0, 0, 5, 0]          # as tests/test_targets_direct_gpu.py


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(g = targets_cases.grid, gt (G,7), bev (G,4,2) f32, abev (N,4,2) f32 in flat anchor order, N)."""
    grid_name, make = CASES[name]
    g = C.grid(grid_name)
    gt = make()
    abev = np.ascontiguousarray(g['bevs'].reshape(-1, 4, 2))
    return dict(g=g, gt=gt, bev=C.bev(gt), abev=abev, N=abev.shape[0])


@functools.lru_cache(maxsize=None)
def truth(name):
    c = case(name)
    return AR.truth_table(c['bev'], c['abev'])


def apart(bev, abev):
    """(G, N) bool: the kernels' bounding-circle test, ground truth first."""
    return R.circles_apart32(np.asarray(bev, np.float32)[:, None], np.asarray(abev, np.float32)[None])


@functools.lru_cache(maxsize=None)
def oracle_table(name):
    """(iou f32 (G, N), stale (G, N) bool): the rule's iou(g, a) from the reference-arithmetic oracle -- 0 where the circles are
    apart, O.bbox_pairwise(ground truth, anchor) otherwise, one pair per call so that ``stale`` marks exactly the pairs on which
    the oracle consumed a scratch slot that an earlier cut left (its value there is not the library's)."""
    c = case(name)
    far = apart(c['bev'], c['abev'])
    iou = np.zeros(far.shape, np.float32)
    stale = np.zeros(far.shape, bool)
    lib = O._oracle_c()
    for g, a in zip(*np.nonzero(~far)):
        before = lib.oracle_anchor_stale_reads()
        iou[g, a] = O.bbox_pairwise(c['bev'][g][None], c['abev'][a][None], True)[0, 0]
        stale[g, a] = lib.oracle_anchor_stale_reads() != before
    return iou, stale


def reference_walk(name, neg=NEG, pos=POS):
    """The reference's classifyAnchors (CPU oracle) on a case: (px, py, pz, nx, ny, nz, gi)."""
    c = case(name)
    nls, nws = C.centre_cells(c['g'], c['gt'])
    pi, ni, gi = O.classify_anchors_cells(c['bev'], c['g']['bevs'], nls, nws, neg, pos)
    return list(pi) + list(ni) + [gi]


def flat(x, y, z, g):
    return (np.asarray(x, np.int64) * g['w'] + np.asarray(y, np.int64)) * g['A'] + np.asarray(z, np.int64)
