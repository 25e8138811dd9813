"""Inputs of the focal-loss tests (tests/test_focal_loss_gpu.py), as numpy arrays in the layout of focal_ref.focal_ref: small
anchor grids with Car-sized anchors, ground truths scattered around them, and index lists whose entries beyond the counts
hold out-of-range garbage (the kernels must never read them)."""
import numpy as np

GARBAGE = 10 ** 9


def anchor_grid(l, w, A):
    """f32 [l][w][A][7] xyzlwhr: a 0.4 m grid of Car anchors (3.9 x 1.6 x 1.56), yaw k * pi / A."""
    an = np.zeros((l, w, A, 7), np.float32)
    an[..., 0] = (np.arange(l, dtype=np.float32) * 0.4 + 0.2)[:, None, None]
    an[..., 1] = (np.arange(w, dtype=np.float32) * 0.4 - 0.2 * w)[None, :, None]
    an[..., 2] = -1.0
    an[..., 3:6] = np.array([3.9, 1.6, 1.56], np.float32)
    an[..., 6] = (np.arange(A, dtype=np.float32) * np.float32(np.pi / A))[None, None, :]
    return an


def boxes(rng, n, l, w):
    """n ground truths f32 (n,7) around the grid, sizes within 20 % of the anchors', any yaw."""
    g = np.zeros((n, 7), np.float32)
    g[:, 0] = rng.uniform(0.0, 0.4 * l, n)
    g[:, 1] = rng.uniform(-0.2 * w, 0.2 * w, n)
    g[:, 2] = rng.uniform(-1.6, -0.4, n)
    g[:, 3:6] = np.array([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.2, (n, 3))
    g[:, 6] = rng.uniform(-1.5, 1.5, n)
    return g


def empty_lists(F, cap):
    pos = np.full((F, 3, cap), GARBAGE, np.int64)
    neg = np.full((F, 3, cap), -GARBAGE, np.int64)
    gi = np.full((F, cap), GARBAGE, np.int64)
    return pos, neg, gi, np.zeros((F, 2), np.int32)


def heads_of(rng, F, l, w, A):
    """Rows [A logits ~ N(0,3) | 7A regression ~ N(0,1.5)]: both SmoothL1 branches occur."""
    h = rng.normal(0.0, 1.5, (F * l * w, 8 * A))
    h[:, :A] = rng.normal(0.0, 3.0, (F * l * w, A))
    return h.astype(np.float32)


def _put(dst, f, entries):
    for k, e in enumerate(entries):
        dst[f, :, k] = e


def case1(seed=1):
    """F=3, l=6, w=5, A=2.  Frame 0: 2 boxes, anchor (1,2,0) twice in pos with different gi, (2,2,0) twice in neg, three
    anchors ignored only; frame 1: counts (0,0); frame 2: no positive, 4 ignored anchors."""
    rng = np.random.default_rng(seed)
    F, l, w, A, cap = 3, 6, 5, 2, 12
    pos, neg, gi, counts = empty_lists(F, cap)
    p0 = [(1, 2, 0), (1, 2, 0), (3, 1, 1), (4, 4, 0)]
    _put(pos, 0, p0)
    gi[0, :4] = [0, 1, 1, 0]
    _put(neg, 0, [(1, 2, 0), (2, 2, 0), (3, 1, 1), (2, 3, 1), (2, 2, 0), (4, 4, 0), (0, 0, 1)])
    counts[0] = (4, 7)
    _put(neg, 2, [(0, 1, 0), (5, 4, 1), (3, 3, 0), (2, 0, 1)])
    counts[2] = (0, 4)
    return dict(F=F, l=l, w=w, A=A, heads=heads_of(rng, F, l, w, A), pos=pos, neg=neg, gi=gi, counts=counts,
                gts=boxes(rng, 3, l, w), gt_off=np.array([0, 2, 2, 3], np.int32), anchors=anchor_grid(l, w, A))


def case2():
    """Case 1 with the logits replaced by a tiling of {-90, -20, 0, 20, 90}: every anchor class meets saturated logits."""
    c = case1()
    heads = c['heads'].copy()
    n = heads.shape[0] * c['A']
    heads[:, :c['A']] = np.resize(np.array([-90, -20, 0, 20, 90], np.float32), n).reshape(-1, c['A'])
    c['heads'] = heads
    return c


def random_case(F, l, w, A, n_pos, n_ign, n_gt, seed):
    """Per frame ``n_pos`` distinct positives (no anchor twice) and ``n_ign`` further anchors listed in neg only."""
    rng = np.random.default_rng(seed)
    cap = n_pos + n_ign + 3
    pos, neg, gi, counts = empty_lists(F, cap)
    for f in range(F):
        pick = rng.permutation(l * w * A)[:n_pos + n_ign]
        xyz = np.stack([pick // (w * A), (pick // A) % w, pick % A])
        pos[f, :, :n_pos] = xyz[:, :n_pos]
        neg[f, :, :n_pos + n_ign] = xyz[:, rng.permutation(n_pos + n_ign)]
        gi[f, :n_pos] = rng.integers(0, n_gt, n_pos)
        counts[f] = (n_pos, n_pos + n_ign)
    return dict(F=F, l=l, w=w, A=A, heads=heads_of(rng, F, l, w, A), pos=pos, neg=neg, gi=gi, counts=counts,
                gts=boxes(rng, n_gt * F, l, w), gt_off=(np.arange(F + 1) * n_gt).astype(np.int32), anchors=anchor_grid(l, w, A))


def case3():
    return random_case(2, 44, 50, 2, 30, 25, 6, seed=3)      # 8,800 float4 pieces per frame: several workgroups, several rounds


def case4():
    return random_case(2, 4, 3, 3, 3, 3, 2, seed=4)          # rows 24 wide


def case5():
    return random_case(16, 2, 3, 2, 2, 2, 1, seed=5)         # MVX_MAX_FRAMES frames
