"""Inputs of the direct detection tests (tests/test_detect_direct_host.py, tests/test_detect_direct_gpu.py): small anchor grids
whose every decoded box is set through the anchors (regression 0: the decoded box is the anchor bit for bit), class logits
built from float32 bit patterns where a digit of the radix select matters, and boxes placed by hand for the mask and the scan.
Everything is numpy from explicit seeds.

A case is a dict: name, grid, l, w, A, F, cls f32 (F, N), reg f32 (F, N, 7), anchors f32 (N, 7) with N = l*w*A and anchor
index n = (x*w + y)*A + a, score_thr, iou_thr, pre_max, post_max, decode, optionally iou f32 (F, N) + alpha (the rectified
score), and what the case claims about itself (checked on the CPU by test_detect_direct_host.py):
    cut      per frame (prefix bits shared by the K-th and (K+1)-th key, deciding byte) or None     selection cases 1 to 3
    ties     per frame dict(m, need, chunks)                                                      selection case 4
    counts   per frame number of candidates                                                       where it is the point
    groups   per frame list of rank tuples: exactly the pairs inside a group overlap                mask and scan cases
    keep     per frame list of the ranks greedy NMS keeps (before post_max)
``order_key`` mirrors bev_iou.h's: it serves the claims only, never an expected result."""
import functools

import numpy as np

GRIDS = {'g35': (5, 7, 1), 'g45': (3, 5, 3), 'g1300': (26, 25, 2), 'g4224': (48, 44, 2), 'g20000': (50, 100, 4)}
BG = np.float32(-10.0)              # sigmoid 4.5e-5: never a candidate at score_thr 0.05
THR = 0.05
CHUNK = 4096                        # keys per trip of detect_select's ordered compaction (1024 threads x 4)
POS, NEG = 0xC0000000, 0x3FFF0000   # keys of the floats 2.0 + r ulp and -2.0 - (65535 - r) ulp


def order_key(x):
    """bev_iou.h order_key in numpy: larger float -> larger u32 key, -0 folded into +0."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).copy()
    u[x == 0] = 0
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_to_float(keys):
    k = np.asarray(keys, np.int64).astype(np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def sort_size(n_sel):
    """P of detect_select's bitonic sort."""
    p = 1
    while p < n_sel:
        p <<= 1
    return p


def spread_anchors(n):
    """(n, 7) 1 m x 1 m boxes 3 m apart (100 per row): no two can touch, every coordinate exact in f32."""
    a = np.zeros((n, 7), np.float32)
    k = np.arange(n)
    a[:, 0], a[:, 1], a[:, 2] = 3.0 * (k % 100), 3.0 * (k // 100), -1.0
    a[:, 3:6] = (1.0, 1.0, 1.5)
    return a


def _case(name, grid, cls, score_thr=THR, pre_max=None, post_max=None, anchors=None, reg=None, **claims):
    l, w, A = GRIDS[grid]
    cls = np.ascontiguousarray(cls, np.float32)
    F, N = cls.shape
    assert N == l * w * A
    c = dict(name=name, grid=grid, l=l, w=w, A=A, F=F, N=N, cls=cls, score_thr=score_thr, iou_thr=0.1, pre_max=pre_max,
             post_max=pre_max if post_max is None else post_max, decode='loss',
             anchors=spread_anchors(N) if anchors is None else np.ascontiguousarray(anchors, np.float32),
             reg=np.zeros((F, N, 7), np.float32) if reg is None else np.ascontiguousarray(reg, np.float32))
    c.update(claims)
    return c


# ---- populations of one frame: (logits (N,), claim) -------------------------------------------------------------------------
def _cut(keys, K, byte):
    """Candidate keys (in anchor order) changed so that the K-th and (K+1)-th largest differ in byte ``byte`` and in no higher
    one: everything below the cut that reaches the K-th key's digit is lowered by whole digits, one key to exactly one less."""
    keys = np.asarray(keys, np.int64).copy()
    order = np.lexsort((np.arange(len(keys)), -keys))
    t, below, sh = keys[order[K - 1]], order[K:], 8 * byte
    assert len(below) and (t >> sh) & 255 >= 1
    b = keys[below]
    while (b >> sh >= t >> sh).any():
        b = np.where(b >> sh >= t >> sh, b - (1 << sh), b)
    b[0] = t - (1 << sh)
    keys[below] = b
    return keys, (int(t) >> (sh + 8) << (sh + 8), byte)


def _scatter(N, where, keys):
    lg = np.full(N, BG, np.float32)
    lg[where] = key_to_float(keys)
    return lg


def pop_digit(N, K, seed, n_cand, span, byte):
    """n_cand > K candidates 2.0 + r ulp, r < span: the keys share their top bits and the cut falls in ``byte``."""
    g = np.random.default_rng(seed)
    where = np.sort(g.choice(N, n_cand, replace=False))
    keys, cut = _cut(POS + g.integers(0, span, n_cand), K, byte)
    return _scatter(N, where, keys), cut


def pop_negative(N, K, seed, n_cand, byte):
    """K // 3 candidates just above 2.0, the rest just below -2.0 (sigmoid 0.119 >= 0.05): the K-th is negative."""
    g = np.random.default_rng(seed)
    where = np.sort(g.choice(N, n_cand, replace=False))
    keys = NEG + g.integers(0, 65536, n_cand)
    up = g.choice(n_cand, K // 3, replace=False)
    keys[up] = POS + g.integers(0, 65536, K // 3)
    keys, cut = _cut(keys, K, byte)
    return _scatter(N, where, keys), cut


def pop_ties(N, K, seed, m, need, low=40):
    """K - need candidates above the key T, m at T exactly, ``low`` below it, all at random anchors."""
    g = np.random.default_rng(seed)
    n_cand = K - need + m + low
    where = g.choice(N, n_cand, replace=False)                      # unsorted: the three kinds interleave in anchor order
    T = POS + 0x1000
    keys = np.concatenate([T + 1 + g.integers(0, 3000, K - need), np.full(m, T), T - 1 - g.integers(0, 3000, low)])
    tied = np.sort(where[K - need:K - need + m])
    return _scatter(N, where, keys), dict(m=m, need=need, chunks=sorted(set((tied // CHUNK).tolist())), tied=tied)


def pop_count(N, seed, count, lo=-2.0, hi=6.0):
    """``count`` candidates with continuous random logits."""
    g = np.random.default_rng(seed)
    lg = np.full(N, BG, np.float32)
    lg[g.choice(N, count, replace=False)] = g.uniform(lo, hi, count).astype(np.float32)
    return lg


# ---- selection and order ------------------------------------------------------------------------------------------------
def _stack(pops):
    return np.stack([p[0] for p in pops]), [p[1] for p in pops]


@functools.lru_cache(maxsize=None)
def selection_cases():
    out = []
    N = 1300
    cls, cut = _stack([pop_digit(N, 300, 11, 700, 256, 0), pop_digit(N, 300, 12, 330, 256, 0), pop_digit(N, 300, 13, 1300, 256, 0)])
    out.append(_case('last_digit', 'g1300', cls, pre_max=300, cut=cut))
    cls, cut = _stack([pop_digit(N, 300, 21, 700, 65536, 1), pop_digit(N, 300, 22, 420, 65536, 1), pop_digit(N, 300, 23, 1300, 65536, 1)])
    out.append(_case('third_digit', 'g1300', cls, pre_max=300, cut=cut))
    cls, cut = _stack([pop_negative(N, 300, 31, 700, 0), pop_negative(N, 300, 32, 450, 1), pop_negative(N, 300, 33, 1300, 0)])
    out.append(_case('kth_negative', 'g1300', cls, pre_max=300, cut=cut))
    cls, ties = _stack([pop_ties(20000, 500, 41, 300, 37), pop_ties(20000, 500, 42, 300, 1), pop_ties(20000, 500, 43, 300, 300),
                        pop_ties(20000, 500, 44, 300, 200)])
    out.append(_case('ties_at_cut', 'g20000', cls, pre_max=500, post_max=100, ties=ties, cut=None))
    counts = [0, 1, 255, 256, 257]
    out.append(_case('population_edges', 'g1300', np.stack([pop_count(N, 50 + k, c) for k, c in enumerate(counts)]), pre_max=256,
                     counts=counts))
    for grid, sizes in (('g1300', (1000, 1024, 1025)), ('g4224', (2048, 2049, 4096))):
        n = np.prod(GRIDS[grid])
        for k in sizes:                                                # frame 0: every anchor (selection), frame 1: exactly k (all)
            out.append(_case('sort_%d' % k, grid, np.stack([pop_count(n, 60 + k, n), pop_count(n, 61 + k, k)]), pre_max=k,
                             counts=[int(n), k], n_sel=k, P=sort_size(k)))
    for grid in ('g35', 'g45'):
        n = int(np.prod(GRIDS[grid]))
        g = np.random.default_rng(70 + n)
        lg = np.stack([g.normal(0.0, 4.0, n), g.normal(-30.0, 40.0, n), -np.abs(g.normal(0.0, 2.0, n))]).astype(np.float32)
        for k in (64, 20):                                             # everything fits / a selection among the n
            out.append(_case('thr0_%s_pre%d' % (grid, k), grid, lg, score_thr=0.0, pre_max=k, counts=[n] * 3))
    return out


NAN_POS, NAN_NEG = np.uint32(0x7fc00000).view(np.float32), np.uint32(0xffc00001).view(np.float32)


@functools.lru_cache(maxsize=None)
def odd_logit_cases():
    """g45, frame 0: -0.0 at anchor 5 and +0.0 at anchor 9; frame 1: the two swapped.  NaNs of both signs at 2, 17 and 44, +inf
    at 30, -inf at 12, the rest random.  Once with score_thr 0 (the -inf is the last candidate) and once with 0.05."""
    g = np.random.default_rng(80)
    base = g.uniform(-2.0, 3.0, 45).astype(np.float32)
    base[base == 0] = 1.0
    base[[2, 17, 44]] = (NAN_POS, NAN_NEG, NAN_POS)
    base[30], base[12] = np.inf, -np.inf
    a, b = base.copy(), base.copy()
    a[5], a[9] = -0.0, 0.0
    b[5], b[9] = 0.0, -0.0
    cls = np.stack([a, b])
    return [_case('odd_thr0', 'g45', cls, score_thr=0.0, pre_max=64, counts=[42, 42]),
            _case('odd_thr0_select', 'g45', cls, score_thr=0.0, pre_max=40, counts=[42, 42]),
            _case('odd_thr05', 'g45', cls, score_thr=THR, pre_max=64, counts=[41, 41])]


KINDS = ('low', 'empty', 'third', 'neg', 'one', 'ties', 'random', 'full', 'empty', 'edge', 'neg', 'low', 'ties', 'third', 'empty',
         'random')


@functools.lru_cache(maxsize=None)
def sixteen_frames():
    """F = 16 on g1300 at pre_max 256: every population above, three frames empty."""
    N, K = 1300, 256
    make = {'low': lambda s: pop_digit(N, K, s, 600, 256, 0)[0], 'third': lambda s: pop_digit(N, K, s, 500, 65536, 1)[0],
            'neg': lambda s: pop_negative(N, K, s, 700, 0)[0], 'ties': lambda s: pop_ties(N, K, s, 200, 9)[0],
            'empty': lambda s: pop_count(N, s, 0), 'one': lambda s: pop_count(N, s, 1), 'random': lambda s: pop_count(N, s, 180),
            'full': lambda s: pop_count(N, s, N), 'edge': lambda s: pop_count(N, s, K + 1)}
    return _case('sixteen', 'g1300', np.stack([make[k](90 + f) for f, k in enumerate(KINDS)]), pre_max=K, post_max=64)


@functools.lru_cache(maxsize=None)
def rectified_case():
    """Selection case 1 with an IoU head at alpha 0.5: class logit 2.0 + r ulp and IoU logit -1 + 0.015 r for r < 256, so equal
    r is an exact tie (the index decides) and different r are >= 4e-4 apart in the log score."""
    N, K = 1300, 300
    cls, iou, cut = [], [], []
    for seed, n_cand in ((11, 700), (12, 330), (13, 1300)):
        lg, c = pop_digit(N, K, seed, n_cand, 256, 0)
        r = order_key(lg).astype(np.int64) - POS
        cls.append(lg)
        iou.append(np.where(lg == BG, BG, np.float32(-1.0) + np.float32(0.015) * r.astype(np.float32)).astype(np.float32))
        cut.append(c)
    return _case('rectified', 'g1300', np.stack(cls), pre_max=K, cut=cut, iou=np.stack(iou), alpha=0.5)


# ---- decode -----------------------------------------------------------------------------------------------------------------
def random_boxes(g, n, lmin=3.0, lmax=5.0, wmin=1.4, wmax=2.0):
    return np.stack([g.uniform(0, 70, n), g.uniform(-40, 40, n), g.uniform(-2, 0, n), g.uniform(lmin, lmax, n),
                     g.uniform(wmin, wmax, n), g.uniform(1.3, 1.9, n), g.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def decode_case():
    """g45 (A = 3): random anchors, regressions ~ N(0, 0.3), every anchor a candidate with a logit in [-2.5, 6]."""
    g = np.random.default_rng(100)
    F, N = 3, 45
    cls = g.uniform(-2.5, 6.0, (F, N)).astype(np.float32)
    return _case('decode', 'g45', cls, pre_max=64, anchors=random_boxes(g, N), reg=g.normal(0.0, 0.3, (F, N, 7)))


# ---- mask and scan: boxes placed by hand --------------------------------------------------------------------------------
SPOT = 10.0                       # metres between the spots of a 16-wide field; the 4 m x 2 m boxes have radius 2.24


def placed(name, frames, pre_max=256, post_max=None, grid='g1300', seed=0, special=None):
    """``frames``: per frame (n ranks, groups).  Rank k sits at an anchor drawn from the seed, with logit 4 - k / 128 (strictly
    decreasing, exact).  A rank outside every group has a spot of its own; the members of a group share the spot of their first
    rank, each a few centimetres (at most 0.26 m in all) further along x.  ``special(f, rank) -> box or None`` overrides."""
    l, w, A = GRIDS[grid]
    N = l * w * A
    g = np.random.default_rng(seed)
    F = len(frames)
    cls = np.full((F, N), BG, np.float32)
    anchors = spread_anchors(N)
    anchors[:, 0] += 1000.0                                            # the unused anchors: far from the field
    rank_anchor, groups_out, keep = [], [], []
    used = g.permutation(N)
    at = 0
    for f, (n, groups) in enumerate(frames):
        mine = used[at:at + n]                                         # every frame has its own anchors: the table is shared
        at += n
        rank_anchor.append(mine)
        cls[f, mine] = (4.0 - np.arange(n) / 128.0).astype(np.float32)
        member = {}
        for grp in groups:
            grp = [r for r in grp if r < n]
            step = min(0.05, 0.26 / max(1, len(grp) - 1))
            for k, r in enumerate(grp):
                assert r not in member
                member[r] = (grp[0], k * step)
        for r in range(n):
            s, dx = member.get(r, (r, 0.0))
            box = (SPOT * (s % 16) + dx, SPOT * (s // 16), -1.0, 4.0, 2.0, 1.5, 0.25 * (s % 4))
            if special is not None and special(f, r) is not None:
                box = special(f, r)
            anchors[mine[r]] = box
        gs = [tuple(r for r in grp if r < n) for grp in groups]
        gs = [t for t in gs if len(t) > 1]
        groups_out.append(gs)
        keep.append([r for r in range(n) if member.get(r, (r, 0))[0] == r])
    return _case(name, grid, cls, pre_max=pre_max, post_max=post_max, anchors=anchors, groups=groups_out, keep=keep,
                 rank_anchor=rank_anchor, n_ranks=[n for n, _ in frames])


WORD_EDGE_SIZES = (1, 2, 63, 64, 65, 128, 129)


@functools.lru_cache(maxsize=None)
def word_edge_case(n):
    """n_sel = n.  Frame 0: rank 0 is overlapped by the ranks {1, 62, 63, 64, 65, n - 1} that exist (they overlap each other
    too: two boxes that each share more than half of a third intersect).  Frames 1 and 2 make single bits decide: frame 1 has
    the pairs (63, 64) -- bit 0 of word 1 in row 63 --, (0, 65) and (1, 62); frame 2 has (62, 63) -- bit 63 of word 0 -- and
    (64, n - 1)."""
    return placed('word_edge_%d' % n, [(n, [(0, 1, 62, 63, 64, 65, n - 1) if n > 66 else (0, 1, 62, 63, 64, 65)]),
                                      (n, [(63, 64), (0, 65), (1, 62)]), (n, [(62, 63), (64, n - 1)] if n > 65 else [(62, 63)])],
                  seed=200 + n)


def _chain_box(f, r):
    """Frame 0 of the mask cases below: rank 10 is 12 m long, ranks 0 and 70 are 6 m boxes over its two ends, 1 m apart."""
    if f != 0 or r not in (0, 10, 70):
        return None
    x, length = {0: (-3.5, 6.0), 10: (0.0, 12.0), 70: (3.5, 6.0)}[r]
    return (300.0 + x, 0.0, -1.0, length, 2.0, 1.5, 0.0)


@functools.lru_cache(maxsize=None)
def scan_cases():
    out = [placed('chunk_removed', [(141, [(3,) + tuple(range(64, 128))]), (141, [])], seed=300)]
    # 0 - 10 and 10 - 70 overlap at IoU 11 / 25; 0 and 70 are disjoint (circles 7 m apart, radii 3.16).  IoU above 0.5 for both
    # is impossible: two boxes that each share more than half of a third intersect each other.
    c = placed('suppressed_suppressor', [(80, []), (80, [(0, 10)])], seed=301, special=_chain_box)
    c['chain'] = [(0, 10), (10, 70)]
    c['keep'][0] = [r for r in range(80) if r != 10]
    out.append(c)
    out.append(_make_identical(placed('identical', [(70, [(5, 6), (63, 64), (20, 21)])], seed=302)))
    return out


def _make_identical(case):
    """The two members of every pair get the same box and the same logit: they tie, the one at the lower anchor index comes
    first and is the kept one."""
    mine = case['rank_anchor'][0]
    for a, b in case['groups'][0]:
        case['anchors'][mine[b]] = case['anchors'][mine[a]]
        case['cls'][0, mine[b]] = case['cls'][0, mine[a]]
        if mine[b] < mine[a]:
            mine[a], mine[b] = mine[b], mine[a]                        # rank a is the lower anchor index
    return case


@functools.lru_cache(maxsize=None)
def post_max_case(post_max):
    """200 disjoint boxes; post_max 64 ends the scan at a chunk edge, 1, 63, 65 and 70 in mid-chunk."""
    return placed('post_max_%d' % post_max, [(200, []), (10, [])], post_max=post_max, seed=303)


POST_MAX = (1, 63, 64, 65, 70)


def _overflow(f, r):
    """Rank 200 of frame 0 and the ranks 201 and 202 share one centre."""
    if r in (200, 201, 202):
        return (150.0, 200.0, -1.0, 4.0, 2.0, 1.5, 0.0)
    return None


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    """210 ranks; frame 0: the regression of rank 200 (lane 3 of the scan) has r3 = 200, exp overflows.  Ranks 201 and 202 are
    coincident with its anchor: 201 is kept, 202 suppressed by 201.  Frame 1 is the same without the overflow: rank 200 is
    kept and takes both."""
    c = placed('nonfinite', [(210, [(201, 202)]), (210, [(200, 201, 202)])], seed=304, special=_overflow)
    c['reg'][0, c['rank_anchor'][0][200], 3] = 200.0
    c['keep'][0] = [r for r in range(210) if r not in (200, 202)]
    c['bad'] = [[200], []]
    return c


@functools.lru_cache(maxsize=None)
def exact_threshold_case():
    """IoU exactly at iou_thr: a 2 m x 2 m box inside a 4 m x 4 m one, both at yaw 0 on small integer coordinates around
    (4, 4): IoU 4 / 16 = 0.25 without a rounding anywhere (further out the origin fan of the clipping rounds, 0.25000238 at
    (20, 40)).  At iou_thr 0.25 'IoU > iou_thr' keeps both.  Frame 1 has the inner box 2 m x 2.5 m (IoU 0.3125): suppressed."""
    def boxes(f, r):
        if r == 2:
            return (4.0, 4.0, -1.0, 4.0, 4.0, 1.5, 0.0)
        if r == 5:
            return (4.0, 4.0, -1.0, 2.0, 2.0 if f == 0 else 2.5, 1.5, 0.0)
        return None
    c = placed('exact_threshold', [(8, []), (8, [])], seed=305, special=boxes)
    c['iou_thr'] = 0.25
    c['keep'] = [list(range(8)), [r for r in range(8) if r != 5]]
    c['exact'] = [(2, 5, 0.25), (2, 5, 0.3125)]
    return c


# ---- full size --------------------------------------------------------------------------------------------------------------
FULL_SEED = 400
BAND = 1e-3


@functools.lru_cache(maxsize=None)
def full_case():
    """g4224 at pre_max = post_max = 4096, F = 2: 4224 random boxes per frame over 70 m x 80 m (2..3 m x 1..1.4 m, any yaw),
    continuous random logits; frame 0 has every anchor a candidate, frame 1 exactly 4096.  A box with a pair whose oracle IoU
    lies within BAND of iou_thr is drawn again (from the same generator) until no pair does; the anchors are shared, so frame
    1 is frame 0's field under other logits."""
    import detect_ref as R
    import mvx_oracle as O
    g = np.random.default_rng(FULL_SEED)
    N = 4224
    boxes = random_boxes(g, N, 2.0, 3.0, 1.0, 1.4)
    quads = R.corners(boxes)
    bad = set()
    for i, (cols, iou) in enumerate(zip(*R.near_pairs(quads))):
        if (np.abs(iou - 0.1) < BAND).any():
            bad.add(i)
    rounds = 0
    while bad:
        rounds += 1
        assert rounds < 50
        at = np.array(sorted(bad))
        boxes[at] = random_boxes(g, len(at), 2.0, 3.0, 1.0, 1.4)
        quads[at] = R.corners(boxes[at])
        ab, ba = O.bbox_pairwise(quads[at], quads, True), O.bbox_pairwise(quads, quads[at], True).T
        ab[np.arange(len(at)), at] = ba[np.arange(len(at)), at] = 1.0
        hit = (np.abs(ab - 0.1) < BAND) | (np.abs(ba - 0.1) < BAND)
        bad = set(at[hit.any(1)].tolist())
    cls = np.stack([pop_count(N, FULL_SEED + 1, N, -2.5, 6.0), pop_count(N, FULL_SEED + 2, 4096, -2.5, 6.0)])
    return _case('full', 'g4224', cls, pre_max=4096, anchors=boxes, counts=[N, 4096])


@functools.lru_cache(maxsize=None)
def near_check_case():
    """600 random car-sized boxes over 70 m x 80 m in random order: greedy_nms_near against greedy_nms."""
    import detect_ref as R
    return R.corners(random_boxes(np.random.default_rng(500), 600))
