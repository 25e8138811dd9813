"""Inputs of the rotated-IoU-loss tests (tests/test_box_iou_loss_host.py, tests/test_box_iou_loss_gpu.py): the smallest shapes
at which the kernel can go wrong.

``pair_case(where, ld)``: F = 3 frames on a 6 x 5 grid with A = 2 anchors per cell (yaw 0 and pi/2, a car's size): frame 0
without a positive (its list slots hold garbage that must never be read), frame 1 with a single positive, frame 2 with 40; cap
= 48 is larger than every count; every entry names its own anchor and its own ground-truth row (gi is a permutation, not the
slot index).  ``where`` = 'near' puts the anchors around the origin, 'far' around x = 69, y = -39 (the far corner of the KITTI
range, where f32 world coordinates have lost 6 bits); ``ld`` = 16 or 20 floats per head row (the plain rows and the rows of a
direction / IoU model).  A ground truth is its anchor moved, resized and turned (any quarter); the regression row is its
encoding plus Gaussian noise, stored in f32.

The pairs are drawn by REJECTION until every frame's quota is full, so none is left out of a comparison afterwards.  Kept are
pairs (b = the float64 decode of the f32 row, g) where the loss is differentiable by a margin:
  * every corner of either rectangle at least MARGIN = 1e-2 m from every edge line of the other,
  * the yaw difference at least 1e-2 rad from a multiple of pi/2,
  * |b2 - g2| and |(b2 + b5) - (g2 + g5)| at least 1e-2,
and, so that every pair has a gradient to compare, a vertical overlap above 5 cm and q above 0.02 (the zeros are edge_case's).

``edge_case()``: one frame on the same grid with anchors and boxes made of dyadic numbers, so that "exactly" means exactly in
f32: a pair that decodes onto its box, the same box half a turn round, boxes that touch along an edge, boxes apart, no vertical
overlap, an overflowing size regression, an anchor outside the grid, gi out of range on both sides, an anchor listed twice.
"""
import functools
import math

import numpy as np

import box_iou_ref as BR
import detect_ref as D
import iou_head_ref as IR

MARGIN = 1e-2
L, W, A = 6, 5, 2
CAP = 48
QUOTA = (0, 1, 40)
ORIGIN = {'near': (-2.0, -1.6), 'far': (67.0, -40.6)}


def anchors_at(x0, y0, pitch=0.8, size=(3.9, 1.6, 1.56), z=-1.0):
    an = np.zeros((L, W, A, 7), np.float32)
    for x in range(L):
        for y in range(W):
            for a in range(A):
                an[x, y, a] = (x0 + pitch * x, y0 + pitch * y, z) + tuple(size) + (a * math.pi / 2,)
    return an


def _line_distances(qa, qb):
    """Distances of the corners of qa from the four edge lines of qb."""
    out = []
    for i in range(4):
        p, e = qb[i], qb[(i + 1) % 4] - qb[i]
        n = np.array([-e[1], e[0]]) / np.hypot(e[0], e[1])
        out.extend(abs(float((c - p) @ n)) for c in qa)
    return out


def violations(b, g):
    """The conditions of the module docstring that the float64 pair (b, g) violates (empty = kept)."""
    bad = []
    qa, qb = IR.quad64(b), IR.quad64(g)
    if min(_line_distances(qa, qb) + _line_distances(qb, qa)) < MARGIN:
        bad.append('a corner within MARGIN of an edge line of the other rectangle')
    turn = (g[6] - b[6]) % (math.pi / 2)
    if min(turn, math.pi / 2 - turn) < MARGIN:
        bad.append('yaw difference within MARGIN of a multiple of pi/2')
    if abs(b[2] - g[2]) < MARGIN or abs((b[2] + b[5]) - (g[2] + g[5])) < MARGIN:
        bad.append('bottom or top faces within MARGIN')
    return bad


def _draw_pair(rng, an):
    g = an.astype(np.float64).copy()
    g[0:2] += rng.normal(0.0, 0.5, 2)
    g[2] += rng.normal(0.0, 0.2)
    g[3:6] *= np.exp(rng.normal(0.0, 0.1, 3))
    g[6] += rng.normal(0.0, 0.3) + rng.integers(-1, 3) * math.pi / 2
    g = g.astype(np.float32)
    r = D.encode(g, an) + rng.normal(0.0, 1.0, 7) * np.array([0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.15])
    return g, r.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _base(where, seed=11):
    """The draw of ``where`` with 16-wide rows; 'drawn' / 'kept' count the rejection.  Read-only: shared between the tests."""
    rng = np.random.default_rng(seed + (0 if where == 'near' else 1))
    F = len(QUOTA)
    an = anchors_at(*ORIGIN[where])
    heads = rng.normal(0.0, 1.0, (F * L * W, 8 * A)).astype(np.float32)
    pos = rng.integers(-9, 99, (F, 3, CAP)).astype(np.int64)           # beyond the counts: garbage, never read
    gi = rng.integers(-9, 99, (F, CAP)).astype(np.int64)
    counts = np.zeros((F, 2), np.int32)
    gt_off = np.zeros(F + 1, np.int32)
    gts, recs, drawn = [], [], 0
    for f, quota in enumerate(QUOTA):
        n_spare = 2 if quota == 0 else 0                                # frame 0 owns boxes that nothing names
        cells = rng.permutation(L * W * A)[:quota]
        rows = rng.permutation(quota)
        frame_gts = [None] * quota
        for k, (cell, row) in enumerate(zip(cells, rows)):
            x, y, z = int(cell) // (W * A), (int(cell) // A) % W, int(cell) % A
            while True:
                drawn += 1
                g, r = _draw_pair(rng, an[x, y, z])
                b = BR.decode64(r, an[x, y, z])
                ih = min(b[2] + b[5], float(g[2]) + float(g[5])) - max(b[2], float(g[2]))
                if not violations(b, g.astype(np.float64)) and ih > 0.05 and IR.iou3d(b, g.astype(np.float64))[0] > 0.02:
                    break
            heads[(f * L + x) * W + y, A + 7 * z:A + 7 * z + 7] = r
            pos[f, :, k] = (x, y, z)
            gi[f, k] = row
            frame_gts[row] = g
            recs.append(dict(f=f, k=k, x=x, y=y, z=z, row=int(gt_off[f]) + int(row)))
        for _ in range(n_spare):
            frame_gts.append(_draw_pair(rng, an[0, 0, 0])[0])
        gts.extend(frame_gts)
        counts[f] = (quota, int(rng.integers(0, CAP)))
        gt_off[f + 1] = gt_off[f] + len(frame_gts)
    return dict(F=F, l=L, w=W, A=A, heads=heads, anchors=an, pos=pos, gi=gi, counts=counts, gts=np.stack(gts).astype(np.float32),
                gt_off=gt_off, recs=recs, drawn=drawn, kept=len(recs))


def widen(case, ld):
    """The case with head rows of ``ld`` floats: further columns hold logits of other heads (here: 7.0)."""
    if ld == case['heads'].shape[1]:
        return case
    wide = np.full((case['heads'].shape[0], ld), 7.0, np.float32)
    wide[:, :case['heads'].shape[1]] = case['heads']
    return dict(case, heads=wide)


@functools.lru_cache(maxsize=None)
def pair_case(where, ld=16):
    return widen(_base(where), ld)


PAIR_CASES = [('near', 16), ('near', 20), ('far', 16), ('far', 20)]
WEIGHT = 0.7              # of the comparisons: not 1, so that a forgotten factor shows
Q_BAR_MAX = 1e-4          # a case's q bar must stay below this ...
GRAD_BAR_MAX = 1e-3       # ... and its gradient bar below this share of the largest reference gradient


@functools.lru_cache(maxsize=None)
def reference(where, ld=16):
    """Computed once per case and shared, never modified: the float64 references (q and out of restatement (a), the gradient of
    restatement (b)) and the bars of the GPU tests -- 4 x the worst distance between the kernel's algorithm restated in f32
    numpy and float64, over the case's own pairs, for q and for the gradient."""
    case = pair_case(where, ld)
    q64, out64 = BR.q_ref(case, WEIGHT)
    _, grad64, _ = BR.loss_autograd(case, WEIGHT)
    q32, _, grad32 = BR.kernel_restated(case, WEIGHT, np.float32)
    taken = q64 >= 0
    worst_q = float(np.abs(q32[taken] - q64[taken]).max())
    worst_g = float(np.abs(grad32.astype(np.float64) - grad64).max())
    return dict(q=q64, out=out64, grad=grad64, worst_q=worst_q, worst_grad=worst_g, q_bar=4.0 * worst_q, grad_bar=4.0 * worst_g,
                grad_max=float(np.abs(grad64).max()))

EDGE_SLOTS = ('exact', 'half_turn', 'touching', 'apart', 'no_vertical', 'overflow', 'outside_grid', 'gi_high', 'gi_negative',
              'twice_a', 'twice_b', 'plain')


@functools.lru_cache(maxsize=None)
def edge_case():
    """One frame, 12 listed entries (EDGE_SLOTS in order), anchors 4 x 2 x 1.5 m with dyadic centres 8 m / 4 m apart."""
    an = np.zeros((L, W, A, 7), np.float32)
    for x in range(L):
        for y in range(W):
            for a in range(A):
                an[x, y, a] = (8.0 + 8.0 * x, -8.0 + 4.0 * y, -1.0, 4.0, 2.0, 1.5, a * math.pi / 2)
    rng = np.random.default_rng(5)
    heads = rng.normal(0.0, 1.0, (L * W, 8 * A)).astype(np.float32)
    pos = np.full((1, 3, 16), -5, np.int64)
    gi = np.full((1, 16), 77, np.int64)
    gts, slots = [], {}

    def put(name, cell, g, r, row=None):
        k = len(slots)
        x, y, z = cell
        pos[0, :, k] = cell
        if 0 <= x < L:
            heads[x * W + y, A + 7 * z:A + 7 * z + 7] = np.asarray(r, np.float32)
        if row is None:
            gts.append(np.asarray(g, np.float32))
            row = len(gts) - 1
        gi[0, k] = row
        slots[name] = k

    zero = np.zeros(7)
    a0 = lambda x, y: an[x, y, 0].astype(np.float64)
    put('exact', (0, 0, 0), a0(0, 0), zero)
    put('half_turn', (1, 0, 0), a0(1, 0) + np.array([0, 0, 0, 0, 0, 0, math.pi]), zero)
    put('touching', (2, 0, 0), a0(2, 0) + np.array([4.0, 0, 0, 0, 0, 0, 0]), zero)              # shares the side x = +l/2
    put('apart', (3, 0, 0), a0(3, 0) + np.array([0, 32.0, 0, 0, 0, 0, 0]), zero)
    put('no_vertical', (4, 0, 0), a0(4, 0) + np.array([0.25, 0, 3.0, 0, 0, 0, 0]), zero)        # BEV overlap, stacked
    put('overflow', (5, 0, 0), a0(5, 0), np.array([0, 0, 0, 100.0, 0, 0, 0]))
    put('outside_grid', (L, 1, 0), a0(0, 1), zero)
    put('gi_high', (0, 2, 0), None, zero, row=40)
    put('gi_negative', (1, 2, 0), None, zero, row=-1)
    g = a0(2, 2) + np.array([0.4, -0.3, 0.1, 0.2, -0.1, 0.1, 0.2])
    r = D.encode(g, an[2, 2, 0]) + np.array([0.05, 0.04, -0.1, 0.1, -0.05, 0.08, -0.1])
    put('twice_a', (2, 2, 0), g, r)
    put('twice_b', (2, 2, 0), None, r, row=gi[0, slots['twice_a']])
    g = a0(3, 3) + np.array([-0.5, 0.2, -0.1, -0.2, 0.1, 0.05, -0.3])
    put('plain', (3, 3, 1), g, D.encode(g, an[3, 3, 1]) + np.array([-0.05, 0.06, 0.1, 0.05, 0.1, -0.08, 0.12]))
    assert tuple(slots) == EDGE_SLOTS
    n = len(slots)
    return dict(F=1, l=L, w=W, A=A, heads=heads, anchors=an, pos=pos, gi=gi, counts=np.array([[n, 3]], np.int32),
                gts=np.stack(gts).astype(np.float32), gt_off=np.array([0, len(gts)], np.int32), slots=slots)
